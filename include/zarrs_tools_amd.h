/*
 * zarrs_tools_amd.h — the C ABI of the MI355X-native zarrs_filter per-chunk transform path.
 *
 * This is the drop-in boundary for the reference's per-chunk filter apply (LDeakin/zarrs_tools
 * 0.7.2, Rust). A Rust host would bind these symbols through a thin `extern "C"` FFI
 * (INTEGRATION.md shows the binding). In this repo the host side above the ABI is Python over
 * ctypes: the zarrs_filter / zarrs_ome drivers (zarrs_tools_amd/zarrs_filter.py, zarrs_ome.py),
 * the tests and the bench; zarrs_tools_amd/csrc/host holds the C++ Zarr V3 store and the
 * overlapped store -> store pipeline behind the zt_store_* entry points.
 *
 * Conventions
 *  - Plain pointers and sizes only. Array buffers are DEVICE pointers (hipMalloc / torch CUDA
 *    tensors) unless a function says otherwise. Shapes/strides are int64 element counts, C order
 *    (last axis fastest), like ndarray's default layout in the reference.
 *  - Every function returns a zt_status (0 = ok, negative = error); the message of the last error
 *    on the calling thread is available from zt_last_error().
 *  - Compute calls are asynchronous on the context's HIP stream; zt_ctx_synchronize() waits.
 *    Contexts are thread-safe across distinct contexts, not re-entrant on one context.
 *  - The library never frees caller memory.
 */
#ifndef ZARRS_TOOLS_AMD_H
#define ZARRS_TOOLS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_ABI_VERSION 4
#define ZT_MAX_DIMS 8

/* Status codes. Negative values mirror FilterError variants (src/filter/filter_error.rs:10-30). */
typedef enum zt_status {
    ZT_OK = 0,
    ZT_ERR_INVALID_PARAMETERS = -1,   /* FilterError::InvalidParameters */
    ZT_ERR_UNSUPPORTED_DATA_TYPE = -2,/* FilterError::UnsupportedDataType (filter.rs:93-101) */
    ZT_ERR_OUT_OF_MEMORY = -3,        /* calculate_chunk_limit "not enough memory" (filter.rs:52-66) */
    ZT_ERR_DEVICE = -4,               /* HIP runtime error (no reference analogue: CPU-only) */
    ZT_ERR_STORAGE = -5,              /* FilterError::StorageError */
    ZT_ERR_ARRAY = -6,                /* FilterError::ArrayError / ArrayCreateError */
    ZT_ERR_IO = -7,                   /* FilterError::IOError */
    ZT_ERR_JSON = -8,                 /* FilterError::JSONError */
    ZT_ERR_INCOMPATIBLE_FILL_VALUE = -9, /* FilterError::IncompatibleFillValue */
    ZT_ERR_OTHER = -10                /* FilterError::Other */
} zt_status;

/* Element types accepted by the filters (guided_filter.rs:203-227, downsample.rs:124-148).
 * Bool is stored as one byte and processed as u8, exactly as the reference's dispatch does
 * (guided_filter.rs:280, downsample.rs:244). bfloat16/float16 are raw 16-bit storage. */
typedef enum zt_dtype {
    ZT_BOOL = 0, ZT_INT8 = 1, ZT_INT16 = 2, ZT_INT32 = 3, ZT_INT64 = 4,
    ZT_UINT8 = 5, ZT_UINT16 = 6, ZT_UINT32 = 7, ZT_UINT64 = 8,
    ZT_BFLOAT16 = 9, ZT_FLOAT16 = 10, ZT_FLOAT32 = 11, ZT_FLOAT64 = 12
} zt_dtype;

typedef struct zt_ctx zt_ctx;

/* ---- library / context ---------------------------------------------------------------------- */

int zt_abi_version(void);
/* Thread-local message of the last error raised on this thread ("" if none). */
const char* zt_last_error(void);
/* Size in bytes of one element of `dtype` (0 for an unknown code). */
size_t zt_dtype_size(int dtype);
/* Number of HIP devices visible (0 on a host without GPUs; never an error). */
int zt_device_count(int* count);
/* One context per (host thread, device): owns a HIP stream, events and reusable scratch. */
int zt_ctx_create(int device, zt_ctx** out);
int zt_ctx_destroy(zt_ctx* ctx);
/* Run subsequent work on an external stream (e.g. torch.cuda.current_stream().cuda_stream).
 * The handle is used verbatim: NULL is the device's default (null) stream.
 * After a switch to a different stream, everything the context issues is ordered after
 * everything it issued before the switch (the new stream waits for an event recorded on the old
 * one: the context's calls share one scratch buffer). A call that sets the stream it already has
 * does nothing. A stream handed to the context is synchronised before it is destroyed: the
 * context cannot order after a stream that no longer exists. */
int zt_ctx_set_stream(zt_ctx* ctx, void* hip_stream);
/* Return to the context's own (non-blocking) stream, the state after zt_ctx_create; a switch
 * like zt_ctx_set_stream's, with the same ordering. */
int zt_ctx_use_own_stream(zt_ctx* ctx);
int zt_ctx_get_stream(zt_ctx* ctx, void** hip_stream);
int zt_ctx_synchronize(zt_ctx* ctx);
/* Device scratch held by the context between calls (staging casts, separable passes): its size,
 * and a release that synchronises the stream and frees it (the next call needing scratch
 * allocates again). Scratch allocation failures return ZT_ERR_OUT_OF_MEMORY. */
int zt_ctx_scratch_bytes(zt_ctx* ctx, uint64_t* bytes);
int zt_ctx_release_scratch(zt_ctx* ctx);
/* Device time in ms of the most recent filter launch recorded on this context (hipEvents around
 * the kernel(s) on the context stream). Valid after zt_ctx_synchronize(). */
int zt_ctx_last_kernel_ms(zt_ctx* ctx, float* ms);

/* ---- operator surface: guided filter -------------------------------------------------------- */

/* GuidedFilter::is_compatible (guided_filter.rs:203-227): ZT_OK or ZT_ERR_UNSUPPORTED_DATA_TYPE. */
int zt_guided_filter_is_compatible(int dtype_in, int dtype_out);
/* GuidedFilter::memory_per_chunk (guided_filter.rs:229-238), bytes for one output chunk. */
int zt_guided_filter_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                      int ndim, uint64_t* bytes);
/* ArraySubsetOverlap::new (array_subset_overlap.rs:11-35) with overlap = 2*radius per axis
 * (guided_filter.rs:88-93): the halo'd input subset of an output subset, clamped to the array,
 * and where the output lies inside it. Host-only, no device work. */
int zt_subset_overlap(const int64_t* array_shape, int ndim, const int64_t* subset_start,
                      const int64_t* subset_shape, const int64_t* overlap,
                      int64_t* input_start, int64_t* input_shape, int64_t* dst_in_src_start);

/*
 * GuidedFilter::apply_ndarray + ArraySubsetOverlap::extract_subset + the TIn->f32 / f32->TOut
 * `as` casts of apply_chunk (guided_filter.rs:98-103, :117-164).
 *   in        : device pointer to the (halo'd) input block of `dtype_in`, shape in_shape[ndim],
 *               element strides in_strides (NULL = C-contiguous). Windows clamp to this block,
 *               as get_block (guided_filter.rs:166-184) clamps to the SAT's shape.
 *   out_start : where the output region starts inside the block (dst_in_src); out_shape its shape.
 *   out       : device pointer, `dtype_out`, shape out_shape, strides out_strides (NULL = C).
 *   epsilon, radius : GuidedFilterArguments (guided_filter.rs:25-33); radius in [0, 127]
 *               (the reference's u8 `radius*2` halo overflows above that).
 * ndim in [1, 8]. 1-3 dims run the fused 2.5-D kernel; 4+ dims run the separable path.
 */
int zt_guided_filter_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                   const int64_t* in_shape, const int64_t* in_strides, int ndim,
                                   const int64_t* out_start, const int64_t* out_shape,
                                   int dtype_out, void* out, const int64_t* out_strides,
                                   float epsilon, int radius);

/*
 * GuidedFilter::apply (guided_filter.rs:240-319) over a device-resident array: every output chunk
 * of the chunk grid [chunk_grid_start, chunk_grid_start + chunk_grid_count) is filtered with its
 * 2r halo read from `in` (the whole array, C-contiguous, shape[ndim]) and written into `out`
 * (same shape, C-contiguous). Pass NULL for the grid range to process every chunk. The chunks are
 * batched into as few launches as the grid allows (one launch for a box of chunks of a 1-3 D
 * array); the result equals the reference's chunk-by-chunk result because every window clamps at
 * the array bounds exactly as the reference's clamped 2r halo makes it.
 */
int zt_guided_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                 void* out, const int64_t* shape, int ndim,
                                 const int64_t* chunk_shape, float epsilon, int radius,
                                 const int64_t* chunk_grid_start,
                                 const int64_t* chunk_grid_count);

/* Multi-GPU z-slab form used by the sharded bench/driver: `in` holds the global rows
 * [in_z0, in_z0 + in_nz) of an array whose full shape is global_shape (C-contiguous slab); the
 * output rows [out_z0, out_z0 + out_nz) (global coordinates, a subset of the input rows, chunk
 * aligned or not) are written into `out` (C-contiguous, out_nz rows). Windows clamp at the global
 * array bounds, so the result equals the reference's per-chunk result for those rows as long as
 * the slab carries a 2r halo (or reaches the array edge). 3-D only. */
int zt_guided_filter_apply_slab(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                void* out, const int64_t* global_shape, int64_t in_z0,
                                int64_t in_nz, int64_t out_z0, int64_t out_nz,
                                const int64_t* chunk_shape, float epsilon, int radius);

/* ---- operator surface: downsample ----------------------------------------------------------- */

/* Downsample::is_compatible (downsample.rs:124-148); discrete requires integer/bool input
 * (downsample.rs:244-256). */
int zt_downsample_is_compatible(int dtype_in, int dtype_out, int discrete);
/* Downsample::output_shape (downsample.rs:162-168): max(shape / stride, 1). */
int zt_downsample_output_shape(const int64_t* in_shape, int ndim, const int64_t* stride,
                               int64_t* out_shape);
/* Downsample::input_subset (downsample.rs:64-70). */
int zt_downsample_input_subset(const int64_t* in_shape, int ndim, const int64_t* stride,
                               const int64_t* out_start, const int64_t* out_shape,
                               int64_t* in_start, int64_t* in_subset_shape);
/*
 * Downsample::apply_ndarray_continuous / apply_ndarray_discrete (downsample.rs:72-120) on a
 * device block: window = min(stride, extent) per axis; only complete windows produce output
 * (exact_chunks); out shape = floor(in_shape / window). Continuous: f64 sum in C order / count,
 * Rust `as` into dtype_out. Discrete (integer/bool input only): the most frequent value, ties
 * broken by the smallest value (documented deterministic rule; the reference's tie order is
 * HashMap iteration order).
 */
int zt_downsample_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                const int64_t* in_shape, int ndim, const int64_t* stride,
                                int discrete, int dtype_out, void* out);

/*
 * zarrs_ome mean pyramid on a device-resident level 0 (zarrs_ome.rs:515-738, levels computed
 * on-device without a store round trip): level i = downsample(level i-1) for i in 1..=max_levels,
 * stopping when every axis has factor 1 or output extent 1 (zarrs_ome.rs:731-737).
 * `level_ptrs[i-1]` receive the levels (device buffers sized by zt_pyramid_level_shapes).
 * Returns the number of levels written through *levels_written.
 */
int zt_pyramid_level_shapes(const int64_t* shape, int ndim, const int64_t* factor, int max_levels,
                            int64_t* level_shapes /* [max_levels][ndim] */, int* n_levels);
int zt_pyramid_downsample(zt_ctx* ctx, int dtype, const void* level0, const int64_t* shape,
                          int ndim, const int64_t* factor, int max_levels, int discrete,
                          void* const* level_ptrs, int* levels_written);

/* ---- synthetic inputs ------------------------------------------------------ */

/* v = 500*[x >= nx/2] + 100*U, U = (splitmix64(seed ^ global_index) >> 40) * 2^-24, written for
 * the global rows [z0, z0 + shape[0]) of an array of shape global_shape (C order, f32). */
int zt_synth_step_noise_f32(zt_ctx* ctx, float* out, const int64_t* shape, int ndim,
                            const int64_t* global_shape, int64_t z0, uint64_t seed);
/* u16 = ((splitmix64(seed ^ global_index) >> 40) * 65535) >> 24. */
int zt_synth_u16(zt_ctx* ctx, uint16_t* out, const int64_t* shape, int ndim,
                 const int64_t* global_shape, int64_t z0, uint64_t seed);
/* The box [start, start + shape) of the N-d global synthetic volume (kind 0: float32 step+noise,
 * kind 1: uint16 noise), element for element the values the whole-array generators give it: a
 * rank generates its own octant / slab of a global array (benchmarks, parity samples). */
int zt_synth_box(zt_ctx* ctx, int kind, void* out, const int64_t* start, const int64_t* shape,
                 const int64_t* global_shape, int ndim, uint64_t seed);

/* Reencode::apply_chunk_convert (src/filter/filters/reencode.rs:58-77): out[i] = in[i].as_() for
 * n contiguous elements of any of the 13 types to any other (num-traits AsPrimitive, half 2.6.0:
 * half types through f32, float -> int saturating with NaN -> 0, int -> int wrapping). Used by
 * zarrs_ome's level 0 with --data-type (zarrs_ome.rs:355-363). */
int zt_reencode_cast(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out, void* out,
                     int64_t n);


/* ---- Gaussian (src/filter/filters/gaussian.rs; src/filter/kernel.rs) ----------------------- */

/* create_sampled_gaussian_kernel (gaussian.rs:252-267): writes the taps (2*half+1, or 1 when
 * sigma == 0) to `taps` (may be NULL to query) and their count to *len. Host only. */
int zt_gaussian_kernel(float sigma, int64_t kernel_half_size, float* taps, int64_t* len);
/* Gaussian::is_compatible (gaussian.rs:123-147): all 13 types in and out. */
int zt_gaussian_is_compatible(int dtype_in, int dtype_out);
/* Gaussian::memory_per_chunk (gaussian.rs:149-168). */
int zt_gaussian_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                 int ndim, const int64_t* kernel_half_size, uint64_t* bytes);
/* Gaussian::apply_ndarray + extract_subset + `as` casts of apply_chunk (gaussian.rs:73-119,
 * kernel.rs:17-73): the separable sampled Gaussian of a C-order device block (per axis, in axis
 * order, f32 sequential tap sums, replicate edges at the block bounds), writing the region
 * [out_start, out_start + out_shape) to `out` (C order, out_shape). sigma / kernel_half_size:
 * ndim entries; kernel_half_size <= 127. Bit-identical to the reference. */
int zt_gaussian_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape,
                              int ndim, const int64_t* out_start, const int64_t* out_shape,
                              int dtype_out, void* out, const float* sigma,
                              const int64_t* kernel_half_size);
/* Gaussian::apply's chunk loop (gaussian.rs:170-249) over a device-resident C-order array: every
 * chunk with its kernel_half_size halo, which equals one pass over the whole array. */
int zt_gaussian_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out, void* out,
                            const int64_t* shape, int ndim, const int64_t* chunk_shape,
                            const float* sigma, const int64_t* kernel_half_size);

/* ---- Gradient magnitude (src/filter/filters/gradient_magnitude.rs; src/filter/kernel.rs) ---- */

/* GradientMagnitudeOperator (gradient_magnitude.rs:24-29). */
enum { ZT_GM_SOBEL = 0, ZT_GM_CENTRAL_DIFFERENCE = 1 };
/* GradientMagnitude::is_compatible (gradient_magnitude.rs:151-175): all 13 types in and out. */
int zt_gradient_magnitude_is_compatible(int dtype_in, int dtype_out);
/* GradientMagnitude::memory_per_chunk (gradient_magnitude.rs:177-195). */
int zt_gradient_magnitude_memory_per_chunk(int dtype_in, int dtype_out,
                                           const int64_t* chunk_shape, int ndim, uint64_t* bytes);
/* GradientMagnitude::apply_ndarray + extract_subset + `as` casts of apply_chunk
 * (gradient_magnitude.rs:91-96, :109-147; kernel.rs:75-129) on a C-order device block: per axis
 * the triangle / difference passes in axis order (Sobel) or one difference pass
 * (CentralDifference), g += s * s, sqrt; replicate edges at the block bounds. Writes the region
 * [out_start, out_start + out_shape) to `out` (C order, out_shape). op: ZT_GM_*. Bit-identical to
 * the reference. 3-D Sobel runs one fused z-march; other ranks and CentralDifference run pass
 * by pass on device scratch. */
int zt_gradient_magnitude_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                        const int64_t* in_shape, int ndim,
                                        const int64_t* out_start, const int64_t* out_shape,
                                        int dtype_out, void* out, int op);
/* GradientMagnitude::apply's chunk loop (gradient_magnitude.rs:197-274) over a device-resident
 * C-order array: every chunk with its halo of 1, which equals one pass over the whole array. */
int zt_gradient_magnitude_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                      void* out, const int64_t* shape, int ndim,
                                      const int64_t* chunk_shape, int op);

/* ---- Rank filters: minimum, median, maximum (an extension; the reference has none) ---------- */

/* Output k selects one element of the window in[clamp(k_a + i_a, 0, n_a - 1)], i_a in
 * [-h_a, h_a] on every axis, h = kernel_half_size (replicate edges, N = prod(2 h_a + 1) entries):
 * the smallest, the entry of rank (N - 1) / 2 of the sorted window, or the largest. Integers order
 * by value, bool false < true, floats by the key bits ^ (sign ? all ones : sign bit) compared
 * unsigned (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN). The result is the selected
 * element's storage bits, unchanged; another output type is its Rust `as` cast. */
enum { ZT_RANK_MINIMUM = 0, ZT_RANK_MEDIAN = 1, ZT_RANK_MAXIMUM = 2 };
/* All 13 types in and out. */
int zt_rank_filter_is_compatible(int dtype_in, int dtype_out);
/* nin * 3 * size_in + nout * (size_in + size_out) with nin = prod(chunk_a + 2 h_a): the input
 * block, two pass buffers and the selected block before the cast. */
int zt_rank_filter_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                    int ndim, const int64_t* kernel_half_size, uint64_t* bytes);
/* The filter of a C-order device block (edges clamp at the block bounds), writing the region
 * [out_start, out_start + out_shape) to `out` (C order, out_shape). kind: ZT_RANK_*;
 * kernel_half_size: ndim non-negative entries; a median window of more than 4096 entries is
 * ZT_ERR_INVALID_PARAMETERS. 3-D blocks with h = (1, 1, 1) and 1/2/4-byte elements run one fused
 * z-march; otherwise minimum / maximum run one pass per axis and the median bisects per output. */
int zt_rank_filter_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                 const int64_t* in_shape, int ndim, const int64_t* out_start,
                                 const int64_t* out_shape, int dtype_out, void* out, int kind,
                                 const int64_t* kernel_half_size);
/* The chunk loop over a device-resident C-order array: every chunk with its kernel_half_size
 * halo, which equals one pass over the whole array. */
int zt_rank_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                               void* out, const int64_t* shape, int ndim,
                               const int64_t* chunk_shape, int kind,
                               const int64_t* kernel_half_size);

/* ---- Summed-area table (src/filter/filters/summed_area_table.rs) ---------------------------- */

/* SummedAreaTable::is_compatible (summed_area_table.rs:110-134): all 13 types in and out. */
int zt_summed_area_table_is_compatible(int dtype_in, int dtype_out);
/* SummedAreaTable::memory_per_chunk (summed_area_table.rs:136-142): one input element plus one
 * output element, as the reference has it (the chunk shape is validated only). */
int zt_summed_area_table_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                          int ndim, uint64_t* bytes);
/* SummedAreaTable::apply_dim for every axis, last to first (summed_area_table.rs:47-106, :172)
 * on a C-order device block: `in as TOut` (:81), then per axis an inclusive running sum,
 * `element += acc` left to right from a zero accumulator in TOut (:69, :94-97). Integer outputs
 * wrap (the reference's release builds; its debug builds panic on overflow). Float outputs keep
 * the reference's order, one rounding to TOut per add, so results are bit-identical. `carry`:
 * NULL, or a device buffer of prod(shape[1:]) TOut elements that holds the seed plane of the
 * axis-0 sum on entry (the reference's sum_last between chunks, :69, :94) and the last output
 * plane on return; NULL seeds with zero. `in` and `out` must not overlap. */
int zt_summed_area_table_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                       const int64_t* shape, int ndim, int dtype_out, void* out,
                                       void* carry);
/* SummedAreaTable::apply's chunk loops (summed_area_table.rs:144-253) over a device-resident
 * C-order array: the carried sums make them one pass per axis over the whole array.
 * `chunk_shape` is validated only. */
int zt_summed_area_table_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                     void* out, const int64_t* shape, int ndim,
                                     const int64_t* chunk_shape);

/* ---- Pointwise filters (src/filter/filters/{reencode,crop,rescale,clamp,equal,replace_value}.rs) */

/* One op of a pointwise program. Op k reads the type op k-1 wrote (the first: the program's
 * input type) and writes `dtype_out`; every `as` is Rust's (zt_reencode_cast's). Per element v:
 *   ZT_PW_REENCODE      v as TOut (Reencode::apply_chunk_convert, reencode.rs:58-88; on a sub-box
 *                       it is Crop::apply_chunk_convert, crop.rs:62-122)
 *   ZT_PW_RESCALE       x = v as f64; fma(x, multiply, add), one rounding, or with
 *                       ZT_PW_ADD_FIRST (x + add) * multiply, two roundings; then `as TOut` from
 *                       f64 (Rescale::apply_elements, rescale.rs:86-122). imm0 / imm1: the f64
 *                       bits of multiply / add.
 *   ZT_PW_CLAMP         lo = min as TIn, hi = max as TIn (f64 -> TIn: saturating, NaN -> 0 for
 *                       integers); v < lo ? lo : (v > hi ? hi : v) (num_traits::clamp: a NaN v
 *                       passes, a NaN bound disables its side); then `as TOut`
 *                       (Clamp::apply_elements, clamp.rs:59-70, :150). imm0 / imm1: the f64 bits
 *                       of min / max.
 *   ZT_PW_EQUAL         (v == value) as TOut, TOut bool or uint8 (Equal::apply_elements,
 *                       equal.rs:62-77, :104-109). imm0: `value` as an element of TIn.
 *   ZT_PW_REPLACE_VALUE v == value ? replace : v as TOut (ReplaceValue::apply_elements,
 *                       replace_value.rs:82-97, :146-153). imm0: `value` as an element of TIn,
 *                       imm1: `replace` as an element of TOut.
 * An element immediate is the element's storage bits, zero-extended (little endian; float16 /
 * bfloat16 raw bits, bool 0 / 1). `==` compares values: -0.0 == 0.0, NaN equals nothing, 64-bit
 * integers exactly. */
enum { ZT_PW_REENCODE = 0, ZT_PW_RESCALE = 1, ZT_PW_CLAMP = 2, ZT_PW_EQUAL = 3,
       ZT_PW_REPLACE_VALUE = 4 };
#define ZT_PW_ADD_FIRST 1 /* zt_pointwise_op.flags: RescaleArguments::add_first (rescale.rs:25-35) */
#define ZT_PW_MAX_OPS 8
typedef struct zt_pointwise_op {
    int32_t kind;      /* ZT_PW_* */
    int32_t dtype_out; /* zt_dtype */
    uint64_t imm0, imm1;
    uint32_t flags;
    uint32_t reserved; /* 0 */
} zt_pointwise_op;

/* is_compatible of the six filters (reencode.rs:92-118, crop.rs:126-150, rescale.rs:126-150,
 * clamp.rs:74-98, equal.rs:81-111, replace_value.rs:101-125): all 13 types in and out; equal
 * writes bool or uint8 only (ZT_ERR_UNSUPPORTED_DATA_TYPE otherwise). kind: ZT_PW_*. */
int zt_pointwise_is_compatible(int kind, int dtype_in, int dtype_out);
/* memory_per_chunk: chunk elements x (input + output element size); for ZT_PW_REENCODE (reencode
 * and crop) the output element size only (reencode.rs:120-126, crop.rs:152-158). */
int zt_pointwise_memory_per_chunk(int kind, int dtype_in, int dtype_out,
                                  const int64_t* chunk_shape, int ndim, uint64_t* bytes);
/* The per-chunk element work of the six filters (Reencode::apply_chunk_convert reencode.rs:58-88,
 * Crop::apply_chunk_convert crop.rs:62-122, Rescale::apply_chunk rescale.rs:68-122,
 * Clamp::apply_elements_inplace clamp.rs:59-70 and the `as` of :150, Equal::apply_elements
 * equal.rs:62-77, ReplaceValue::apply_elements replace_value.rs:82-97) for a program of n_ops in
 * [1, ZT_PW_MAX_OPS] ops in one launch: the box [sub_start, sub_start + sub_shape) of the C-order
 * device array `in` (dtype_in, in_shape[ndim]; both NULL: the whole array) goes through the ops
 * in order, every intermediate `as` performed, into `out` (C order, sub_shape, the last op's
 * dtype_out), so the result is bit-identical to the ops run one call at a time. The type chain is
 * validated like zt_pointwise_is_compatible. `in` and `out` need element alignment only. A box
 * with a zero extent is a no-op. */
int zt_pointwise_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape,
                               int ndim, const int64_t* sub_start, const int64_t* sub_shape,
                               const zt_pointwise_op* ops, int n_ops, void* out);

/* ---- two-array arithmetic (an extension: the reference has no such filter) ------------------- */

/* out[i] = (first[i] as f64  op  second[i] as f64) as TOut. `as` is Rust's (64-bit integers round
 * to nearest even, half types convert exactly, bool is 0 / 1); op is one IEEE f64 operation, no
 * contraction, denormals kept; the final cast is rescale's (float -> integer saturates, NaN -> 0,
 * f64 -> half in one rounding, bool written as uint8). minimum is `y < x ? y : x` and maximum
 * `y > x ? y : x`: a NaN on either side, or +-0 against -+0, returns x. */
enum { ZT_AR_ADD = 0, ZT_AR_SUBTRACT = 1, ZT_AR_MULTIPLY = 2, ZT_AR_DIVIDE = 3,
       ZT_AR_MINIMUM = 4, ZT_AR_MAXIMUM = 5, ZT_AR_ABSOLUTE_DIFFERENCE = 6 };
/* All 13 types for each of the three arrays, independently; an unknown op is
 * ZT_ERR_INVALID_PARAMETERS. */
int zt_arithmetic_is_compatible(int op, int dtype_a, int dtype_b, int dtype_out);
/* memory_per_chunk: chunk elements x the sum of the three element sizes. */
int zt_arithmetic_memory_per_chunk(int op, int dtype_a, int dtype_b, int dtype_out,
                                   const int64_t* chunk_shape, int ndim, uint64_t* bytes);
/* n contiguous device elements of each array, on the context's stream. The pointers need element
 * alignment only, each on its own; `out` must not overlap `a` or `b`. n == 0 is a no-op. */
int zt_arithmetic_apply(zt_ctx* ctx, int op, int dtype_a, const void* a, int dtype_b,
                        const void* b, int64_t n, int dtype_out, void* out);

/* ---- connected-component labelling (an extension: the reference has no such filter) ---------- */

/* labels[i] = 0 where in[i] is background, else the number 1 .. K of i's component. An element is
 * foreground when its value is not zero: any bit set for bool and the integers (all 64 bits of
 * the 8-byte types), value != 0 for the four float types (+-0.0 are background; NaNs, subnormals
 * and infinities are foreground). Two foreground elements are neighbours when their coordinates
 * differ by at most 1 on every axis and on at most `connectivity` axes (1 = faces, ndim = the
 * full 3^ndim - 1 neighbourhood; nothing wraps at the array edges); a component is a class of the
 * transitive closure, and components are numbered in the C order of their first elements, as
 * scipy.ndimage.label numbers them. Semantics and kernels: DESIGN.md §3.13. */
/* The tile of the three innermost axes that one workgroup labels in LDS. */
#define ZT_CC_TILE_Z 8
#define ZT_CC_TILE_Y 8
#define ZT_CC_TILE_X 64
/* An extension. All 13 types in; the eight integer types out (bool and the float types are
 * ZT_ERR_UNSUPPORTED_DATA_TYPE). */
int zt_connected_components_is_compatible(int dtype_in, int dtype_out);
/* An extension. Device bytes of one call: input + scratch + output. Scratch is two index arrays,
 * 2 * n * 4 bytes (2 * n * 8 when n >= 2^32 - 1 or ZT_CC_INDEX64=1), and a tail of
 * 64 + 16 * (3^ndim - 1) / 2 bytes (K and the offset table). 0 for an array with a zero extent. */
int zt_connected_components_memory(int dtype_in, int dtype_out, const int64_t* shape, int ndim,
                                   uint64_t* bytes);
/* An extension. Labels the whole C-order device array `in` (shape[ndim], element alignment) into
 * `out` (same shape, dtype_out, element alignment, not overlapping `in`) on the context's stream
 * and returns K in *count (may be NULL). connectivity outside [1, ndim] is
 * ZT_ERR_INVALID_PARAMETERS. When K exceeds dtype_out's maximum the call fails with
 * ZT_ERR_INVALID_PARAMETERS (`connected_components: K components do not fit TYPE`) and `out` is
 * not written: labels never wrap. The call synchronises the stream once, to read K before it
 * writes. A refused scratch allocation is ZT_ERR_OUT_OF_MEMORY. A zero extent is a no-op with
 * K = 0. There is no per-chunk form: a component may span every chunk. */
int zt_connected_components_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                        void* out, const int64_t* shape, int ndim,
                                        int connectivity, uint64_t* count);

/* ---- exact Euclidean distance transform (an extension: the reference has no such filter) ------ */

/* out[p] = the Euclidean distance from p to the nearest background element, or its square. The
 * foreground rule is the labelling's: any bit set for bool and the integers, value != 0 for the
 * four float types. spacing[a] >= 1 is the length of one step along axis a (NULL = all ones), and
 *     d2(p) = min over background q of sum_a spacing[a]^2 * (p[a] - q[a])^2,
 * an integer; 0 for a background element, +inf everywhere when the array has no background
 * element; nothing wraps or replicates at the array edges. With squared == 0 the stored element is
 * sqrt(d2 as f64) (correctly rounded) as TOut, the Rust `as` cast: saturating and truncating for
 * integers, round-to-nearest-even for floats, +inf -> the type's maximum / +inf. With squared != 0
 * it is d2 saturated at the maximum of an integer TOut, (d2 as f64) as TOut for a float TOut.
 * With B = sum_a spacing[a]^2 * (shape[a] - 1)^2 the device works in uint32_t when B < 2^32 - 1
 * and in uint64_t from there on (or with ZT_EDT_WORK64=1, read at every call); B >= 2^62, more
 * than 2^38 elements or an extent >= 2^31 are ZT_ERR_INVALID_PARAMETERS, and so is a spacing
 * below 1. Semantics and kernels: DESIGN.md §3.14. */
/* An extension. All 13 types in; the 12 numeric types out (bool is
 * ZT_ERR_UNSUPPORTED_DATA_TYPE). */
int zt_distance_transform_is_compatible(int dtype_in, int dtype_out);
/* An extension. Device bytes of one call: input + scratch + output,
 *     n * (size(dtype_in) + size(dtype_out)) + n * (2 * W + 8),
 * W = 4 or 8 the work width that shape, spacing and ZT_EDT_WORK64 select: two work arrays (an
 * axis pass reads one and writes the other) and the apex and breakpoint stacks, 4 bytes per
 * element each. 0 for an array with a zero extent. */
int zt_distance_transform_memory(int dtype_in, int dtype_out, const int64_t* shape,
                                 const int64_t* spacing /* NULL = ones */, int ndim,
                                 uint64_t* bytes);
/* An extension. Transforms the whole C-order device array `in` (shape[ndim], element alignment)
 * into `out` (same shape, dtype_out, element alignment, not overlapping `in`) on the context's
 * stream, without synchronising it. A refused scratch allocation is ZT_ERR_OUT_OF_MEMORY. A zero
 * extent is a no-op. There is no per-chunk form: the nearest background element may lie in any
 * chunk. */
int zt_distance_transform_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                      void* out, const int64_t* shape, const int64_t* spacing,
                                      int ndim, int squared);

/* ---- per-label statistics and the label size filter (extensions: no reference operation) ------ */

/* A label array holds 0 for background and 1 .. K for objects (what zt_connected_components
 * writes). The statistics are a reduction keyed by label into a device `state` of u64 words,
 * struct-of-arrays over K + 1 rows: column c of label l is word c * (K + 1) + l (row 0, the
 * background, is never written).
 *   column 0                  count: the elements of the label
 *   columns 1 + 3a .. 3 + 3a  on axis a: the smallest coordinate, the largest (inclusive) and the
 *                             sum of the coordinates, coordinates being those of the whole array
 *                             (origin + index in the box)
 *   with an intensity array, after the ndim axes:
 *   column 1 + 3 ndim         the smallest orderable key of the label's non-NaN intensities
 *   column 2 + 3 ndim         the largest
 *   columns 3, 4 + 3 ndim     the sum of the intensities as a 128-bit two's complement integer
 *                             (lo, hi), kept for the six integer types of up to 32 bits
 *   word cols * (K + 1)       the number of label elements outside [0, K]
 * An absent label has count 0, minima of all ones and maxima of 0; a label with no non-NaN
 * intensity has a smallest key above its largest. The key of an element is its storage bits
 * (zero-extended) for the unsigned types, with the sign bit flipped for the signed ones, and for the
 * float types the bits with the sign bit set when it was clear and all bits flipped when it was
 * set: keys order as the values do, -0.0 below +0.0, the infinities as values. Every column is an
 * integer sum, minimum or maximum: the state does not depend on the launch geometry, and
 * accumulating two halves of an array equals accumulating the whole. Limits, all
 * ZT_ERR_INVALID_PARAMETERS: K in [0, 2^31 - 2]; at most 2^38 elements in a box; origin >= 0;
 * elements * (largest origin + extent) < 2^64, so that no coordinate sum wraps. Semantics and
 * kernels: DESIGN.md §3.15. */
#define ZT_NO_DTYPE (-1) /* dtype_intensity of a call without an intensity array */
/* The rows of a tile of the statistics kernel (a tile is ZT_LABELS_TILE_ROWS rows x 64 x). */
#define ZT_LABELS_TILE_ROWS 16
/* An extension. Labels: the eight integer types; intensity: ZT_NO_DTYPE or the 12 numeric types
 * (anything else is ZT_ERR_UNSUPPORTED_DATA_TYPE). */
int zt_label_statistics_is_compatible(int dtype_labels, int dtype_intensity);
/* An extension. Bytes of the state: 8 * ((1 + 3 ndim + (with_intensity ? 4 : 0)) * (K + 1) + 1). */
int zt_label_statistics_state_bytes(int ndim, int64_t n_labels, int with_intensity,
                                    uint64_t* bytes);
/* An extension. Fills `state` (device memory, 8-byte aligned) with the empty state on the
 * context's stream. */
int zt_label_statistics_init(zt_ctx* ctx, int ndim, int64_t n_labels, int with_intensity,
                             void* state);
/* An extension. Folds the contiguous C-order device box `labels` (box_shape[ndim], element
 * alignment) that lies at `origin` (NULL = zeros) of the whole array into `state` on the context's
 * stream, without synchronising it. `intensity` (same shape, dtype_intensity, element alignment)
 * goes with a state that was sized and initialised with_intensity; NULL with ZT_NO_DTYPE
 * otherwise. An element below 0 or above n_labels is counted in the state's last word and changes
 * nothing else. A zero extent is a no-op. The grid is capped (ZT_LABELS_MAX_BLOCKS lowers the cap,
 * ZT_LABELS_LDS_SLOTS the slots of a workgroup's table; both are read at every call). */
int zt_label_statistics_accumulate(zt_ctx* ctx, int dtype_labels, const void* labels,
                                   int dtype_intensity, const void* intensity,
                                   const int64_t* box_shape, const int64_t* origin, int ndim,
                                   int64_t n_labels, void* state);
/* An extension. Waits for the stream and copies the state into host_state (host memory of
 * zt_label_statistics_state_bytes; may be NULL). When elements outside [0, K] were counted the
 * call fails with ZT_ERR_INVALID_PARAMETERS (`label_statistics: N elements outside [0, K]`);
 * *invalid (may be NULL) receives N either way. */
int zt_label_statistics_finish(zt_ctx* ctx, const void* state, int ndim, int64_t n_labels,
                               int with_intensity, uint64_t* host_state, uint64_t* invalid);

/* The label size filter: a label whose count lies in [min_size, max_size] is kept, every other
 * label becomes 0. With relabel != 0 the kept labels are renumbered 1 .. K' in increasing order of
 * their old value (so the output of zt_connected_components stays numbered in the C order of first
 * elements); otherwise they keep their values. *kept receives K', the number of labels kept. */
/* An extension. The eight integer types in and out. */
int zt_label_size_filter_is_compatible(int dtype_in, int dtype_out);
/* An extension. Device bytes of one call on an array whose largest label is n_labels: input +
 * scratch + output, n * (size(dtype_in) + size(dtype_out)) + 8 * (K + 2) +
 * round_up(4 * (K + 1), 8) + 16 (the counts and their trailing word, the remap table, K' and the
 * largest label kept). 0 for an array with a zero extent. */
int zt_label_size_filter_memory(int dtype_in, int dtype_out, const int64_t* shape, int ndim,
                                int64_t n_labels, uint64_t* bytes);
/* An extension. Filters the whole C-order device array `in` (shape[ndim], element alignment) into
 * `out` (same shape, dtype_out, element alignment, not overlapping `in`) on the context's stream.
 * min_size < 1, max_size < min_size (max_size < 0 = no upper bound), a negative element, a
 * largest label above 2^31 - 2 and a largest output label that does not fit dtype_out are
 * ZT_ERR_INVALID_PARAMETERS, all before `out` is written. The call synchronises the stream twice:
 * to read the largest label, then K' and the check of the elements. A zero extent is a no-op with
 * K' = 0. */
int zt_label_size_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                     void* out, const int64_t* shape, int ndim, int64_t min_size,
                                     int64_t max_size, int relabel, uint64_t* kept);

/* ---- morphological reconstruction (an extension: the reference has no such filter) ------------- */

/* Reconstruction of a marker under a mask, both of one shape and one element type. Elements are
 * only selected, under the rank filters' total order (unsigned and signed integer order, false <
 * true, floats -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN): every output element carries
 * the storage bits of some marker or mask element. Two elements are neighbours when their
 * coordinates differ by at most 1 on every axis and on at most `connectivity` axes (nothing wraps
 * or replicates at the edges). By dilation: J0 = min(marker, mask) (a marker above the mask is
 * clipped, not an error) and out is the least J >= J0 with J[p] = min(max(J[q] : q = p or a
 * neighbour of p), mask[p]) for every p. By erosion: the same with the order reversed. The marker
 * modes other than ZT_REC_MARKER make the marker from the mask on the device: ZT_REC_FILL_HOLES
 * (by erosion; the mask where any coordinate is 0 or extent - 1, the type's greatest key
 * elsewhere), ZT_REC_H_MAXIMA (by dilation; (mask as f64 - h) as T, the arithmetic filter's
 * subtract) and ZT_REC_H_MINIMA (by erosion; (mask as f64 + h) as T). Semantics, kernels and the
 * termination argument: DESIGN.md §3.16. */
/* The tile of the three innermost axes that one workgroup of a round owns, and the rounds the host
 * launches between two reads of their flag words. */
#define ZT_REC_TILE_Z 8
#define ZT_REC_TILE_Y 8
#define ZT_REC_TILE_X 32
#define ZT_REC_BATCH 8
enum { ZT_REC_DILATION = 0, ZT_REC_EROSION = 1 };
enum { ZT_REC_MARKER = 0, ZT_REC_FILL_HOLES = 1, ZT_REC_H_MAXIMA = 2, ZT_REC_H_MINIMA = 3 };
/* An extension. All 13 types; a marker type other than the mask's (read with ZT_REC_MARKER only)
 * and bool with the two h modes are ZT_ERR_UNSUPPORTED_DATA_TYPE; an unknown marker mode is
 * ZT_ERR_INVALID_PARAMETERS. */
int zt_reconstruction_is_compatible(int dtype_mask, int dtype_marker, int marker_mode);
/* An extension. Device bytes of one call: input(s) + scratch + output = n * size for the mask, as
 * much again for a marker array (ZT_REC_MARKER only) and for the output, and the scratch: one
 * working array of n * size bytes rounded up to 16, and 64 bytes of flag words. 0 for an array
 * with a zero extent. A rank that the call refuses (below) is ZT_ERR_INVALID_PARAMETERS here
 * too. */
int zt_reconstruction_memory(int dtype, int marker_mode, const int64_t* shape, int ndim,
                             uint64_t* bytes);
/* An extension. Reconstructs on the whole C-order device arrays `mask` and `marker` (shape[ndim],
 * element alignment; `marker` is read with ZT_REC_MARKER only and may be NULL otherwise) into
 * `out` (same shape and type, not overlapping them) on the context's stream. `method` (ZT_REC_
 * DILATION / EROSION) counts with ZT_REC_MARKER only; `h` (finite, > 0) with the two h modes only.
 * connectivity outside [1, ndim], a rank above 3 with an axis in front of the innermost three
 * whose extent is not 1, more than 2^38 elements or 2^31 - 1 tiles are
 * ZT_ERR_INVALID_PARAMETERS, before anything is written. Rounds alternate between `out` and the
 * scratch array, ZT_REC_BATCH at a time, each with its own flag word; the call synchronises the
 * stream once per batch to read the flags, and stops at the first round that changed nothing
 * (*rounds, may be NULL, counts it). ZT_REC_TILE_SWEEPS=N (read at every call) caps the sweeps of a
 * tile per round; more than n + 1 rounds are ZT_ERR_OTHER. A refused scratch allocation is
 * ZT_ERR_OUT_OF_MEMORY. A zero extent is a no-op with 0 rounds. There is no per-chunk form. */
int zt_reconstruction_apply_array(zt_ctx* ctx, int dtype, const void* mask, const void* marker,
                                  int marker_mode, double h, void* out, const int64_t* shape,
                                  int ndim, int connectivity, int method, uint64_t* rounds);

/* ---- seeded watershed (an extension: the reference has no such filter) ------------------------- */

/* The marker-controlled watershed of a relief from the non-zero elements of a seeds array of the
 * same shape. The relief is compared only through the rank filters' total order (above), with the
 * keys complemented when `descending` (a distance map flooded from its maxima); labels are carried
 * as storage bits and never computed on. The domain D is every element, or with `foreground_only`
 * every element whose relief is not zero by the labelling's rule; elements outside D get 0, are
 * never crossed, and a seed there is ignored. Neighbours are reconstruction's. (1) c[p] is the
 * least, over paths in D from a seed to p, of the greatest key on the path. (2) d[p] is 0 at seeds
 * and where a D-neighbour has a smaller c, else 1 + the least d over D-neighbours of equal c; no d
 * exists exactly where no seed is connected to p in D, and such elements get 0. (3) The parent of
 * p is p at a seed; for d = 0 the D-neighbour of least (c, linear C index) among those with a
 * smaller c; for d > 0 the neighbour of least linear index with equal c and d one less.
 * (4) labels[p] = seeds[root of p]. The result is unique. Semantics, kernels and the termination
 * argument: DESIGN.md §3.18. */
/* An extension. A relief of any of the 13 types and seeds of one of the 8 integer types; anything
 * else is ZT_ERR_UNSUPPORTED_DATA_TYPE. */
int zt_watershed_is_compatible(int dtype_relief, int dtype_seeds);
/* An extension. Device bytes of one call: inputs + output + scratch = n * size(relief) +
 * 2 * n * size(seeds) + the scratch, every part of it rounded up to 16 bytes: two working arrays
 * of n * size(relief) for the pass values, a third for the relief copy with `foreground_only`,
 * two arrays of 4 n bytes (the plateau distances, then the parents), and 64 bytes of flag words.
 * 0 for an array with a zero extent. What the call refuses for the connectivity, the rank or the
 * size (below) is ZT_ERR_INVALID_PARAMETERS here too. */
int zt_watershed_memory(int dtype_relief, int dtype_seeds, const int64_t* shape, int ndim,
                        int connectivity, int foreground_only, uint64_t* bytes);
/* An extension. The watershed of the whole C-order device arrays `relief` and `seeds`
 * (shape[ndim], element alignment) into `out` (the seeds' type, not overlapping them) on the
 * context's stream. connectivity outside [1, ndim], a rank above 3 with an axis in front of the
 * innermost three whose extent is not 1, 2^32 - 1 elements or more, or more than 2^31 - 1 tiles
 * are ZT_ERR_INVALID_PARAMETERS, before anything is written. Pass values are reconstruction's
 * rounds, distances rounds of the same tile, jumps P' = P[P]; all are launched ZT_REC_BATCH at a
 * time with one flag word each, the call synchronises the stream once per batch, and a phase stops
 * at its first round that changed nothing. rounds (may be NULL) receives the pass rounds, the
 * distance rounds and the jumps, each counting that last round. ZT_REC_TILE_SWEEPS=N caps the
 * sweeps of a tile per round in both tiled phases. More than n + 1 pass or distance rounds or
 * ceil(log2 n) + 2 jumps are ZT_ERR_OTHER; a refused scratch allocation is ZT_ERR_OUT_OF_MEMORY.
 * A zero extent is a no-op with 0 rounds. There is no per-chunk form. */
int zt_watershed_apply_array(zt_ctx* ctx, int dtype_relief, const void* relief, int dtype_seeds,
                             const void* seeds, void* out, const int64_t* shape, int ndim,
                             int connectivity, int descending, int foreground_only,
                             int64_t rounds[3]);

/* ---- zarrs_info reductions (src/info/range.rs, src/info/histogram.rs) ------------------------ */

/* The 12 numeric types; ZT_BOOL is ZT_ERR_UNSUPPORTED_DATA_TYPE (the reference reaches
 * `unimplemented!` there, range.rs:92-95, histogram.rs:32-35). */
int zt_range_is_compatible(int dtype);
int zt_histogram_is_compatible(int dtype);
/* The range of an array (calculate_range, range.rs:99-131, with the meaning its documentation
 * gives it: the smallest and the largest element; as written the reference seeds min with the
 * type's minimum and max with its maximum, :113-116, so neither moves). Integers are compared
 * exactly; NaN elements are ignored (PartialOrd, :115-116); -0.0 orders below +0.0; the
 * infinities are values. `state` is 16 bytes of device memory, 8-byte aligned, that accumulates
 * across calls: zt_range_init empties it, zt_range_accumulate folds n contiguous device elements
 * (element alignment; n == 0 is a no-op) into it on the context's stream. */
int zt_range_init(zt_ctx* ctx, void* state);
int zt_range_accumulate(zt_ctx* ctx, int dtype, const void* in, int64_t n, void* state);
/* Waits for the stream and reads the state back: *none = 1 when no non-NaN element was folded
 * (min_bits / max_bits are then 0), else the smallest and largest element as storage bits of
 * `dtype`, zero-extended (as zt_pointwise_op's element immediates). */
int zt_range_finish(zt_ctx* ctx, int dtype, const void* state, uint64_t* min_bits,
                    uint64_t* max_bits, int* none);
/* calculate_histogram's per-element work (histogram.rs:51-68): for every one of n contiguous
 * device elements x, in f64 with one rounding per operation,
 *   norm = (x as f64 - min) / (max - min);  bin = min(floor(max(norm * n_bins, 0)) as usize,
 *   n_bins - 1)
 * and hist[bin] += 1 on the device array hist (uint64[n_bins], which the caller zeroes; calls
 * accumulate). NaN elements and the 0 / 0 of max == min land in bin 0, +inf in the last bin.
 * n_bins in [1, 2^30], min and max finite, or ZT_ERR_INVALID_PARAMETERS (the reference
 * underflows n_bins - 1 at n_bins == 0). n == 0 is a no-op. */
int zt_histogram_accumulate(zt_ctx* ctx, int dtype, const void* in, int64_t n, int64_t n_bins,
                            double min, double max, uint64_t* hist);
/* bin_edges[i] = (i as f64 / n_bins as f64) * (max - min) + min for i in 0..=n_bins
 * (histogram.rs:62-68), n_bins + 1 host doubles. Host only. */
int zt_histogram_bin_edges(int64_t n_bins, double min, double max, double* edges);

/* ---- zarrs_validate comparison (src/bin/zarrs_validate.rs) ----------------------------------- */

/* The per-element work of zarrs_validate (`bytes_first == bytes_second`, zarrs_validate.rs:
 * 145-147): two contiguous device runs of n elements of one data type (all 13 types) compared by
 * their storage bits, so a NaN equals a NaN with the same bits only, +0.0 differs from -0.0 and
 * bool is a byte. `state` is 16 bytes of device memory, 8-byte aligned, that accumulates across
 * calls: the number of differing elements and the smallest differing element index.
 * zt_compare_init empties it; zt_compare_accumulate folds a and b (element alignment, which may
 * differ between the two; n == 0 is a no-op) into it on the context's stream, an element's index
 * being `base` (>= 0) plus its index in the run. */
int zt_compare_init(zt_ctx* ctx, void* state);
int zt_compare_accumulate(zt_ctx* ctx, int dtype, const void* a, const void* b, int64_t n,
                          int64_t base, void* state);
/* Waits for the stream and reads the state back: *n_diff the number of differing elements,
 * *first the smallest differing index, -1 when the runs were equal (zarrs_validate.rs:147). */
int zt_compare_finish(zt_ctx* ctx, const void* state, uint64_t* n_diff, int64_t* first);

/* ---- chunk occupancy (zarrs `store_empty_chunks = false`; Zarr V3 sharding specification) ----- */

/* Which cells of a box hold anything but the fill value. zarrs' `store_empty_chunks` option
 * (default false) makes Array::store_chunk erase a chunk whose elements all equal the fill value
 * (FillValue::equals_all, a comparison of the elements' bytes) instead of writing it, and the
 * sharding codec leave such an inner chunk out of the shard; the Zarr V3 sharding specification
 * (sharding_indexed, "Binary shard format") marks it with offset and nbytes of 2^64 - 1 in the
 * shard index. This is that test for a whole device-resident box at once: `data` is a contiguous
 * C-order box of `shape` (ndim <= ZT_MAX_DIMS, element alignment) of any of the 13 data types,
 * tiled from its origin by cells of `cell_shape` (extents >= 1; the last cell of an axis may be
 * partial, a cell may be larger than the box); `fill_bits` holds the fill value's storage bits,
 * zero-extended little endian. occupied (device memory, one byte per cell, C order of the cell
 * grid ceil(shape / cell_shape)) becomes 1 where some element's bits differ from the fill
 * value's, else 0: a NaN fill matches only its own payload, +0.0 is not -0.0, bool is a byte.
 * Runs on the context's stream; a box with a zero extent has no cells and launches nothing. */
int zt_chunk_occupancy_is_compatible(int dtype);
int zt_chunk_occupancy(zt_ctx* ctx, int dtype, const void* data, const int64_t* shape, int ndim,
                       const int64_t* cell_shape, uint64_t fill_bits, uint8_t* occupied);

/* ---- Zarr V3 store -> store path (host storage in and out) ----------------------------------
 * The reference's filters read and write Zarr arrays through zarrs (Array::retrieve_array_subset_
 * ndarray / store_array_subset_ndarray, guided_filter.rs:95-110; zarrs_ome.rs:226-232). These
 * entry points restate that I/O for filesystem stores (zarr.json V3 metadata, regular chunk grid,
 * default/v2 chunk keys, codecs bytes, gzip, zstd (runtime libzstd.so.1), crc32c and
 * sharding_indexed) and drive the device kernels over it with a pipelined chunk-row loop:
 * decode (host threads) -> H2D -> kernel -> D2H -> encode (host threads), each input chunk
 * decoded once. Host buffers here are ordinary host memory. */

/* Per-call statistics (the reference's Progress read/process/write split, progress.rs:15-105,
 * plus the device phases). *_s of host phases are thread-seconds; device phases are event
 * seconds summed over chunk rows; wall_s is the whole call. */
typedef struct zt_store_stats {
    double wall_s;
    double decode_s, encode_s;         /* host thread-seconds: read+decode, encode+write */
    double h2d_s, kernel_s, d2h_s;     /* device seconds */
    uint64_t bytes_read, bytes_written;/* encoded bytes moved to/from storage */
    uint64_t voxels;                   /* output elements produced */
    int64_t rows;                      /* output chunk rows processed */
    int threads;                       /* host worker threads used */
    int rows_in_flight;                /* input chunk rows held decoded (memory-bounded) */
    int double_buffered;               /* 1: device slabs / output rows double buffered */
} zt_store_stats;

/* Per-chunk progress of the store filters (Progress / ProgressCallback, progress.rs:15-119):
 * after every output chunk is written, `fn` receives the step count, the number of steps (output
 * chunks of the call) and the cumulative read (decode thread-seconds), process (device seconds)
 * and write (encode thread-seconds) durations. Called from the host worker threads, serialised;
 * process-wide; NULL disables. */
typedef struct zt_progress {
    int64_t step, num_steps;
    double read_s, process_s, write_s;
} zt_progress;
typedef void (*zt_progress_fn)(const zt_progress* progress, void* user);
void zt_store_set_progress_callback(zt_progress_fn fn, void* user);

/* --chunk-limit (zarrs_ome.rs:136-141; GuidedFilter::apply's chunk_limit, guided_filter.rs:
 * 251-258): the store filters called afterwards FROM THIS THREAD hold at most `max_chunks` chunks
 * in flight (decoded input rows + output rows being computed or encoded) and use at most that many
 * host worker threads; the pipeline never goes below one input slab and one output row without
 * overlap (a chunk row is its unit of device work). 0 (the default) = bounded by memory only.
 * Replaces the reference's per-filter `chunk_limit` argument. */
int zt_store_set_chunk_limit(int64_t max_chunks);

/* zarrs' `store_empty_chunks` option for the store filters and writes made afterwards FROM THIS
 * THREAD. 1 (the default here; the reference's default is false) stores every chunk. 0 elides
 * chunks that hold nothing but the fill value, as the reference's stores do: a cell (a chunk, or
 * an inner chunk of a shard) is empty when the storage bits of every element inside the array's
 * shape equal the fill value's; an empty chunk of an unsharded array is not written and an
 * existing file of it is removed; an empty inner chunk adds no bytes to its shard and both words
 * of its index entry are 2^64 - 1 (Zarr V3 sharding specification), the other inner chunks stay
 * contiguous; a shard of empty inner chunks is not written and an existing file is removed. An
 * elided chunk still is a progress step and adds 0 to bytes_written; zarr.json does not change.
 * The store filters find the empty cells on the device (zt_chunk_occupancy on every output row
 * before it is copied out); writes from host data scan on the host. A thread starts with 0
 * instead of 1 when the environment has ZT_STORE_EMPTY_CHUNKS=0 (worker processes inherit the
 * setting that way). */
int zt_store_set_store_empty_chunks(int store_empty_chunks);
/* The chunks (files: chunks of an unsharded array, shards) and the inner chunks inside the
 * array's inner-chunk grid (of an unsharded array: its chunks) that the last store filter or
 * write called from this thread elided. Either pointer may be NULL. */
int zt_store_last_elided(int64_t* chunks, int64_t* inner_chunks);

/* flags for the store filters */
#define ZT_STORE_ERASE_OUTPUT_METADATA 1 /* remove OUT/zarr.json first ("not finished" marker,
                                             zarrs_filter.rs:297-300) */
#define ZT_STORE_FINISH_OUTPUT 2         /* write OUT/zarr.json at the end (zarrs_filter.rs:313) */

/* Array metadata of a Zarr V3 array: data type (zt_dtype), rank, shape, chunk (= shard) shape and
 * the inner chunk shape of a sharded array (= chunk shape otherwise). Arrays of ZT_MAX_DIMS. */
int zt_store_array_info(const char* path, int* dtype, int* ndim, int64_t* shape,
                        int64_t* chunk_shape, int64_t* inner_chunk_shape);
/* Create an array and write its zarr.json. codecs_json: a Zarr V3 codec list (NULL = [bytes,
 * little endian]); fill_value_json: Zarr V3 fill_value JSON (NULL = 0 / false / 0.0). */
int zt_store_create_array(const char* path, int dtype, int ndim, const int64_t* shape,
                          const int64_t* chunk_shape, const char* codecs_json,
                          const char* fill_value_json);
/* The output array the filters create: the input's shape, chunking and codecs with data type
 * dtype_out (-1 = the input's) and the input fill value cast to it (filter_traits.rs:47-82). */
int zt_store_create_output_like(const char* in_path, const char* out_path, int dtype_out,
                                const char* encoding_json);
/* The output array of a filter step with an explicit output shape (NULL = the input's): what the
 * store filters create before they run (the downsample output is max(n / stride, 1), so
 * Downsample::output_shape, downsample.rs:162-168), with the same reencoding. Used to give
 * device-resident run-config chains (zarrs_filter.rs:338-381) the arrays the store path would
 * have made, without writing the intermediate data. */
int zt_store_create_output(const char* in_path, const char* out_path, int dtype_out,
                           const int64_t* out_shape, int ndim, const char* encoding_json);
/* Read any subset into a C-order host buffer (missing chunks read as the fill value). */
int zt_store_read_subset(const char* path, const int64_t* start, const int64_t* shape,
                         void* host_out, int nthreads);
/* Write a chunk-aligned subset (may end at the array edge) from a C-order host buffer. */
int zt_store_write_subset(const char* path, const int64_t* start, const int64_t* shape,
                          const void* host_in, int nthreads);
/* zt_store_write_subset with a map the caller already has (zt_chunk_occupancy of the same data
 * with the array's inner chunk shape as the cell shape, copied to the host): occupied_host holds
 * one byte per inner chunk of the subset, C order of ceil(shape / inner chunk shape), 0 = empty.
 * It is consulted when this thread's store_empty_chunks setting is 0, in place of the host scan;
 * NULL = decide on the host. The data of a cell whose byte is 0 is not read; host_in may be NULL
 * when the setting is 0 and the whole map is 0 (the subset's chunk files are removed). */
int zt_store_write_subset_occupancy(const char* path, const int64_t* start, const int64_t* shape,
                                    const void* host_in, const uint8_t* occupied_host,
                                    int nthreads);
/* Fill an existing array with the SURVEY.md §8(d) synthetic data (kind 0: float32 step+noise,
 * kind 1: uint16 noise), identical to zt_synth_step_noise_f32 / zt_synth_u16. */
int zt_store_write_synth(const char* path, int kind, uint64_t seed, int nthreads);

/* encoding_json (NULL or "" = the input's encoding): a JSON object with the reencoding
 * arguments of the filter commands (ZarrReencodingArgs, lib.rs:274-377; applied as
 * get_array_builder_reencode, lib.rs:408-650): "data_type", "fill_value", "separator",
 * "chunk_shape", "shard_shape", "array_to_array_codecs" (only []), "array_to_bytes_codec" (bytes),
 * "bytes_to_bytes_codecs" (gzip / zstd / crc32c), "dimension_names", "attributes",
 * "attributes_append". A "data_type" there takes precedence over dtype_out. Output arrays whose
 * chunk rows do not fit 80 % of the available host / device memory (with no overlap) fail with
 * ZT_ERR_OUT_OF_MEMORY, as calculate_chunk_limit does (filter.rs:52-66). */
/* zarrs_filter guided-filter IN OUT EPS R [--data-type T] over a store (GuidedFilter::apply,
 * guided_filter.rs:240-319): the output array is IN's shape/chunking/codecs with dtype_out (-1 =
 * input type). Processes the output chunk rows [row_begin, row_end) along axis 0 (row_end < 0 =
 * all), so ranks can split the rows; the array's zarr.json is written only with
 * ZT_STORE_FINISH_OUTPUT. nthreads <= 0: min(16, hardware threads). stats may be NULL. */
int zt_store_guided_filter(const char* in_path, const char* out_path, int dtype_out,
                           const char* encoding_json, float epsilon, int radius, int device,
                           int64_t row_begin, int64_t row_end, int nthreads, int flags,
                           zt_store_stats* stats);
/* zt_store_guided_filter restricted to the output chunk columns [col_begin, col_end) along
 * axis 1 (col_end < 0: all), the input read with the 2r halo along axes 0 and 1: one process's
 * (t, z) block of a multi-GPU split (config T; the reference's per-chunk loop,
 * guided_filter.rs:260-316, over that block's chunks). */
int zt_store_guided_filter_box(const char* in_path, const char* out_path, int dtype_out,
                               const char* encoding_json, float epsilon, int radius, int device,
                               int64_t row_begin, int64_t row_end, int64_t col_begin,
                               int64_t col_end, int nthreads, int flags, zt_store_stats* stats);
/* zarrs_filter downsample / one zarrs_ome level over a store (Downsample::apply,
 * downsample.rs:170-286): output shape max(n / stride, 1), encoding as the input's with the
 * encoding_json overrides (zarrs_ome passes its per-level chunk / shard shapes). */
int zt_store_downsample(const char* in_path, const char* out_path, const int64_t* stride,
                        int discrete, int dtype_out, const char* encoding_json, int device,
                        int64_t row_begin, int64_t row_end, int nthreads, int flags,
                        zt_store_stats* stats);
/* zarrs_filter gaussian IN OUT SIGMA HALF [--data-type T] over a store (Gaussian::apply,
 * gaussian.rs:170-249): as zt_store_guided_filter, halo = kernel_half_size. */
int zt_store_gaussian(const char* in_path, const char* out_path, int dtype_out,
                      const char* encoding_json, const float* sigma,
                      const int64_t* kernel_half_size, int device, int64_t row_begin,
                      int64_t row_end, int nthreads, int flags, zt_store_stats* stats);
/* zarrs_filter gradient-magnitude IN OUT [--operator OP] [--data-type T] over a store
 * (GradientMagnitude::apply, gradient_magnitude.rs:197-274): as zt_store_guided_filter, halo 1;
 * op: ZT_GM_*. */
int zt_store_gradient_magnitude(const char* in_path, const char* out_path, int dtype_out,
                                const char* encoding_json, int op, int device, int64_t row_begin,
                                int64_t row_end, int nthreads, int flags, zt_store_stats* stats);
/* zarrs_filter median | minimum | maximum IN OUT KERNEL_HALF_SIZE [--data-type T] over a store:
 * as zt_store_guided_filter, halo = kernel_half_size; kind: ZT_RANK_* (another value is
 * ZT_ERR_INVALID_PARAMETERS). */
int zt_store_rank_filter(const char* in_path, const char* out_path, int dtype_out,
                         const char* encoding_json, int kind, const int64_t* kernel_half_size,
                         int device, int64_t row_begin, int64_t row_end, int nthreads, int flags,
                         zt_store_stats* stats);
/* zarrs_filter summed-area-table IN OUT [--data-type T] over a store (SummedAreaTable::apply,
 * summed_area_table.rs:144-253) in one read and one write of the store (the reference: one of
 * each per axis): every chunk row along axis 0 is summed along its other axes on its own, and
 * the axis-0 sum takes the previous row's last plane from a device buffer. The rows depend on
 * each other in order, so there is no row range. Progress counts each output chunk once, not
 * once per axis (:152-159). */
int zt_store_summed_area_table(const char* in_path, const char* out_path, int dtype_out,
                               const char* encoding_json, int device, int nthreads, int flags,
                               zt_store_stats* stats);
/* zarrs_filter reencode / crop / rescale / clamp / equal / replace-value over a store (the apply
 * chunk loops: reencode.rs:128-218, crop.rs:164-247, rescale.rs:160-239, clamp.rs:108-211,
 * equal.rs:125-214, replace_value.rs:135-240), or several of them in one pass: the program
 * `ops` (zt_pointwise_apply_ndarray) runs on every output chunk row, no halo. crop_offset /
 * crop_shape (both NULL: no crop; one entry per axis, inside the input or
 * ZT_ERR_INVALID_PARAMETERS) make the output the box's shape (Crop::output_shape,
 * crop.rs:160-162), output element i reading input element crop_offset + i
 * (get_input_output_subset, crop.rs:62-76). The output array's data type (dtype_out /
 * encoding_json, as zt_store_guided_filter) must be the last op's dtype_out; missing input
 * chunks read as the fill value and go through the ops like any element. Rows as
 * zt_store_guided_filter. */
int zt_store_pointwise(const char* in_path, const char* out_path, int dtype_out,
                       const char* encoding_json, const zt_pointwise_op* ops, int n_ops,
                       const int64_t* crop_offset, const int64_t* crop_shape, int device,
                       int64_t row_begin, int64_t row_end, int nthreads, int flags,
                       zt_store_stats* stats);
/* zarrs_filter arithmetic over two stores: out = first op second (zt_arithmetic_apply) on every
 * chunk row of the first array, no halo. The shapes must be equal (ZT_ERR_INVALID_PARAMETERS,
 * `Array shapes do not match: [..] vs [..]`, before any device work); the second array may have
 * another data type, chunk grid, sharding and codecs: for every row the chunks of the second
 * array that meet the row's planes are decoded into a row of the same shape, so a chunk of the
 * second array taller than a row is decoded once per row it meets (as zt_store_compare). The
 * output array is built from the first array (dtype_out < 0: the first array's type;
 * encoding_json as zt_store_guided_filter). Missing chunks of either array read as that array's
 * fill value and go through the operator. Rows as zt_store_guided_filter; the host and device
 * budgets and the chunk limit count both inputs; progress counts output chunks. */
int zt_store_arithmetic(const char* first_path, const char* second_path, const char* out_path,
                        int dtype_out, const char* encoding_json, int op, int device,
                        int64_t row_begin, int64_t row_end, int nthreads, int flags,
                        zt_store_stats* stats);
/* One zarrs_ome level with --gaussian-sigma (apply_chunk_continuous_gaussian, zarrs_ome.rs:
 * 236-271): the Gaussian of each downsample input subset (plus its kernel_half_size halo), then
 * the mean downsample of that f32 block to the level's data type. */
int zt_store_downsample_gaussian(const char* in_path, const char* out_path, const int64_t* stride,
                                 const float* sigma, const int64_t* kernel_half_size,
                                 int dtype_out, const char* encoding_json, int device,
                                 int64_t row_begin, int64_t row_end, int nthreads, int flags,
                                 zt_store_stats* stats);
/* zarrs_info PATH range / histogram N_BINS MIN MAX over a store (zarrs_info.rs:170-197;
 * calculate_range range.rs:99-131, calculate_histogram histogram.rs:37-75): the decode -> H2D
 * ring of the filters with no output array, the reduction of zt_range_accumulate /
 * zt_histogram_accumulate on every input chunk row [row_begin, row_end) along axis 0 (row_end
 * < 0 = all) and one small D2H at the end. Only the elements inside the array's shape count (the
 * reference also counts the stored padding of edge chunks, retrieve_chunk_elements, range.rs:112,
 * histogram.rs:54); a chunk absent from the store counts as its fill value. Results over disjoint
 * row ranges combine to the whole: histograms add, ranges fold. Progress counts input chunks.
 * zt_store_range: *dtype the array's type, the rest as zt_range_finish. zt_store_histogram:
 * hist is n_bins host uint64, overwritten. */
int zt_store_range(const char* path, int device, int64_t row_begin, int64_t row_end, int nthreads,
                   int* dtype, uint64_t* min_bits, uint64_t* max_bits, int* none,
                   zt_store_stats* stats);
int zt_store_histogram(const char* path, int64_t n_bins, double min, double max, int device,
                       int64_t row_begin, int64_t row_end, int nthreads, uint64_t* hist,
                       zt_store_stats* stats);
/* zarrs_validate FIRST SECOND over two stores (zarrs_validate.rs:90-157). Shape, then data type
 * are checked before any device work: ZT_ERR_INVALID_PARAMETERS with the reference's messages
 * `Array shapes do not match: [..] vs [..]` and `Array data types do not match: A vs B`
 * (:101-113); encoding and attributes are ignored. Then the decode -> H2D ring of zt_store_range
 * with two inputs: for every chunk row [row_begin, row_end) of the FIRST array along axis 0
 * (row_end < 0 = all) the chunks of both arrays that meet the row are decoded into two rows of
 * one shape (a chunk of the second array taller than a row is decoded once per row it meets, as
 * retrieve_array_subset per first-array chunk does, :146) and compared by zt_compare_accumulate.
 * Only the elements inside the shape count; a chunk absent from a store counts as that array's
 * fill value. *n_diff is the number of differing elements, *first the C-order index in the whole
 * array of the first of them, -1 when there is none. Results over disjoint row ranges combine to
 * the whole: counts add, the first index is the minimum. Progress counts the chunks of both
 * arrays. */
int zt_store_compare(const char* first_path, const char* second_path, int device,
                     int64_t row_begin, int64_t row_end, int nthreads, uint64_t* n_diff,
                     int64_t* first, zt_store_stats* stats);
/* 1 if the named codec can be read and written here, else 0. */
int zt_store_codec_available(const char* name);
/* Host bytes the store pipeline budgets 80 % of (the available-memory half of
 * calculate_chunk_limit, filter.rs:52-66): ZT_STORE_HOST_MEMORY if set, else MemAvailable capped
 * at the cgroup's limit minus its usage net of reclaimable (inactive) page cache. */
uint64_t zt_store_host_available_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* ZARRS_TOOLS_AMD_H */
