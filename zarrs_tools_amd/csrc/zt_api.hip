// zt_api.hip — the C ABI (include/zarrs_tools_amd.h): validation, geometry and launches.
//
// Host-side restatement of the reference's per-chunk orchestration around the kernels:
//   chunk_subset_bounded + ArraySubsetOverlap::new/extract_subset (guided_filter.rs:87-103,
//   array_subset_overlap.rs:11-51), Downsample::input_subset/output_shape (downsample.rs:64-70,
//   :162-168), is_compatible/memory_per_chunk (guided_filter.rs:203-238, downsample.rs:124-160),
//   and the zarrs_ome level loop's shapes and stop rule (zarrs_ome.rs:515-560, :731-737).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zarrs_tools_amd.h"
#include "zt_device.hpp"
#include "zt_edt_host.hpp"
#include "zt_kernels.hpp"
#include "zt_labels_host.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(ZT_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

#define ZT_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess) return hip_fail(_e, #call);                                        \
    } while (0)

bool valid_dtype(int d) { return d >= ZT_BOOL && d <= ZT_FLOAT64; }

const char* dtype_name(int d) {
    static const char* names[] = {"bool",   "int8",   "int16",    "int32",   "int64",
                                  "uint8",  "uint16", "uint32",   "uint64",  "bfloat16",
                                  "float16", "float32", "float64"};
    return valid_dtype(d) ? names[d] : "unknown";
}

}  // namespace

struct zt_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t cur = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_switch = nullptr;  // orders a new stream after the one it replaces
    bool issued = false;    // an entry point has run since the last switch: `cur` may hold work
    bool recorded = false;  // ev_switch has been recorded: earlier work may still be pending
    bool timed = false;
    void* scratch = nullptr;
    size_t scratch_bytes = 0;

    int ensure_scratch(size_t bytes) {
        if (bytes <= scratch_bytes) return ZT_OK;
        if (scratch) {
            (void)hipStreamSynchronize(cur);
            (void)hipFree(scratch);
            scratch = nullptr;
            scratch_bytes = 0;
        }
        hipError_t e = hipMalloc(&scratch, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ZT_ERR_OUT_OF_MEMORY, "device scratch of %zu bytes: %s", bytes,
                        hipGetErrorString(e));
        }
        scratch_bytes = bytes;
        return ZT_OK;
    }
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int now = -1;
        if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
    }
};

int check_ctx(zt_ctx* ctx) {
    if (!ctx) return fail(ZT_ERR_INVALID_PARAMETERS, "null context");
    return ZT_OK;
}

// The first step of every entry point that issues work on the context's stream (or hands the
// stream out): check_ctx, and a note that the current stream may hold the context's work from now
// on (switch_stream).
int begin_call(zt_ctx* ctx) {
    if (int rc = check_ctx(ctx)) return rc;
    ctx->issued = true;
    return ZT_OK;
}

int check_shape(const int64_t* shape, int ndim, const char* what) {
    if (ndim < 1 || ndim > ZT_MAX_DIMS)
        return fail(ZT_ERR_INVALID_PARAMETERS, "%s: ndim %d not in [1, %d]", what, ndim,
                    ZT_MAX_DIMS);
    if (!shape) return fail(ZT_ERR_INVALID_PARAMETERS, "%s: null shape", what);
    for (int d = 0; d < ndim; ++d)
        if (shape[d] < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "%s: negative extent", what);
    return ZT_OK;
}

int64_t numel(const int64_t* s, int n) {
    int64_t r = 1;
    for (int i = 0; i < n; ++i) r *= s[i];
    return r;
}

void c_strides(const int64_t* shape, int ndim, int64_t* strides) {
    int64_t s = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        strides[d] = s;
        s *= shape[d];
    }
}

int radius_ok(int radius) {
    if (radius < 0 || radius > zt::kMaxRadius)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "radius %d not in [0, %d] (the reference's u8 halo radius*2 overflows)", radius,
                    zt::kMaxRadius);
    return ZT_OK;
}

int dtypes_ok(int dtype_in, int dtype_out) {
    if (!valid_dtype(dtype_in))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype_in);
    if (!valid_dtype(dtype_out))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype_out);
    return ZT_OK;
}

// The fused kernel addresses each z-plane through a buffer descriptor with 32-bit byte offsets
// (gf_fused.hpp: slice_rsrc, int row strides): every input plane and output plane it touches must
// span < 2^31 bytes, measured after the f32 staging run_fused3 may insert. Larger planes go to
// the separable path (64-bit indexing) instead of silently reading zeros past the range.
bool fused_planes_fit(const int64_t dom[3], int64_t in_sy, const int64_t oshape[3],
                      int64_t out_sy, int dtype_in, int dtype_out) {
    const bool stage_in = !zt::fused_direct_pair(dtype_in, zt::kF32);
    const bool stage_out = !zt::fused_direct_pair(zt::kF32, dtype_out);
    const int64_t isy = stage_in ? dom[2] : in_sy, osy = stage_out ? oshape[2] : out_sy;
    const int64_t iesz = stage_in ? 4 : (int64_t)zt::dtype_size(dtype_in);
    const int64_t oesz = stage_out ? 4 : (int64_t)zt::dtype_size(dtype_out);
    const int64_t lim = (int64_t)INT32_MAX - 16;  // + one quad of slack past the last element
    if (dom[1] <= 0 || dom[2] <= 0 || oshape[1] <= 0 || oshape[2] <= 0) return true;
    const int64_t ib = ((dom[1] - 1) * isy + dom[2]) * iesz;
    const int64_t ob = ((oshape[1] - 1) * osy + oshape[2]) * oesz;
    return ib <= lim && ob <= lim && dom[1] <= INT32_MAX && dom[2] <= INT32_MAX &&
           dom[0] <= INT32_MAX;
}

// Fused launch on a 3-D view (pad 1-2 D arrays with leading unit axes).
int run_fused3(zt_ctx* ctx, int dtype_in, const void* in, const int64_t dom[3], int64_t in_z0,
               int64_t in_rows, int64_t in_sz, int64_t in_sy, const int64_t ostart[3],
               const int64_t oshape[3], int dtype_out, void* out, int64_t out_sz, int64_t out_sy,
               float eps, int radius, int chunk_depth) {
    for (int d = 0; d < 3; ++d)
        if (dom[d] > INT32_MAX || oshape[d] > INT32_MAX)
            return fail(ZT_ERR_INVALID_PARAMETERS, "extent exceeds 2^31-1");
    if (!fused_planes_fit(dom, in_sy, oshape, out_sy, dtype_in, dtype_out))
        return fail(ZT_ERR_INVALID_PARAMETERS, "fused path: a z-plane spans >= 2 GiB");
    zt::GFParams p{};
    p.in = in;
    p.out = out;
    p.in_sz = in_sz;
    p.in_sy = in_sy;
    p.out_sz = out_sz;
    p.out_sy = out_sy;
    p.in_z0 = (int)in_z0;
    p.zlo = (int)std::max<int64_t>(0, in_z0);
    p.zhi = (int)std::min<int64_t>(dom[0], in_z0 + in_rows);
    p.nz = (int)dom[0];
    p.ny = (int)dom[1];
    p.nx = (int)dom[2];
    p.oz0 = (int)ostart[0];
    p.oy0 = (int)ostart[1];
    p.ox0 = (int)ostart[2];
    p.onz = (int)oshape[0];
    p.ony = (int)oshape[1];
    p.onx = (int)oshape[2];
    p.eps = eps;
    if (p.onz == 0 || p.ony == 0 || p.onx == 0) return ZT_OK;
    // Pairs without a direct instantiation: stage the input rows and/or the output region
    // through contiguous f32 scratch (cast kernels with the same Rust `as` semantics).
    const bool stage_in = !zt::fused_direct_pair(dtype_in, zt::kF32);
    const bool stage_out = !zt::fused_direct_pair(zt::kF32, dtype_out);
    const int64_t in_elems = stage_in ? in_rows * dom[1] * dom[2] : 0;
    const int64_t out_elems = stage_out ? oshape[0] * oshape[1] * oshape[2] : 0;
    if (stage_in || stage_out) {
        int rc = ctx->ensure_scratch(sizeof(float) * (size_t)(in_elems + out_elems));
        if (rc) return rc;
    }
    float* sin = static_cast<float*>(ctx->scratch);
    float* sout = sin + in_elems;
    if (stage_in) {
        hipError_t e = zt::launch_cast_to_f32_3d(in, dtype_in, in_sz, in_sy, sin, in_rows, dom[1],
                                                 dom[2], ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "input staging cast");
        p.in = sin;
        p.in_sz = dom[1] * dom[2];
        p.in_sy = dom[2];
        dtype_in = zt::kF32;
    }
    if (stage_out) {
        p.out = sout;
        p.out_sz = oshape[1] * oshape[2];
        p.out_sy = oshape[2];
    }
    // every launch decision (gf_plan.hpp), on the geometry and element types actually launched
    const int dt_out = stage_out ? (int)zt::kF32 : dtype_out;
    const zt::FusedGeom geom{p.ny, p.nx, p.oy0, p.ox0, p.onz, p.ony, p.onx,
                             p.in_sz, p.in_sy, p.out_sz, p.out_sy};
    const zt::FusedPlan plan =
        zt::plan_fused(geom, radius, (int)zt::dtype_size(dtype_in), (int)zt::dtype_size(dt_out),
                       (uintptr_t)p.in, (uintptr_t)p.out, chunk_depth);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_guided_fused(p, plan, dtype_in, dt_out, radius, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "guided filter fused kernel launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (stage_out) {
        e = zt::launch_cast_from_f32_3d(sout, dtype_out, out, out_sz, out_sy, oshape[0],
                                        oshape[1], oshape[2], ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "output staging cast");
    }
    return ZT_OK;
}

int run_separable(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* shape,
                  const int64_t* in_strides, int ndim, const int64_t* out_start,
                  const int64_t* out_shape, int dtype_out, void* out, const int64_t* out_strides,
                  float eps, int radius) {
    zt::NdGeom g{};
    g.ndim = ndim;
    g.numel = numel(shape, ndim);
    g.out_numel = numel(out_shape, ndim);
    for (int d = 0; d < ndim; ++d) {
        g.shape[d] = shape[d];
        g.in_strides[d] = in_strides[d];
        g.out_start[d] = out_start[d];
        g.out_shape[d] = out_shape[d];
        g.out_strides[d] = out_strides[d];
    }
    if (g.numel == 0 || g.out_numel == 0) return ZT_OK;
    int rc = ctx->ensure_scratch(sizeof(float) * (size_t)zt::separable_scratch_floats(g.numel));
    if (rc) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_guided_separable(in, dtype_in, out, dtype_out, g, radius, eps,
                                               static_cast<float*>(ctx->scratch), ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "guided filter separable launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

// 4-D blocks (config T): guided4d.hip when the radius fits it and x is the unit-stride axis;
// the scratch holds U3/S3, AB and (for other element types or strides) f32 v.
bool use_guided4d(int ndim, int radius, const int64_t* in_strides, const int64_t* shape) {
    return ndim == 4 && zt::guided4d_supports(radius) && in_strides[3] == 1 && shape[0] <= 32 &&
           shape[1] <= 0x7FFFFFFF && shape[2] <= 65535 && shape[3] <= 0x7FFFFFFF;
}

int run_guided4d(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* shape,
                 const int64_t* in_strides, const int64_t* out_start, const int64_t* out_shape,
                 int dtype_out, void* out, const int64_t* out_strides, float eps, int radius) {
    zt::NdGeom g{};
    g.ndim = 4;
    g.numel = numel(shape, 4);
    g.out_numel = numel(out_shape, 4);
    for (int d = 0; d < 4; ++d) {
        g.shape[d] = shape[d];
        g.in_strides[d] = in_strides[d];
        g.out_start[d] = out_start[d];
        g.out_shape[d] = out_shape[d];
        g.out_strides[d] = out_strides[d];
        if (shape[d] > INT32_MAX) return fail(ZT_ERR_INVALID_PARAMETERS, "extent exceeds 2^31-1");
    }
    if (g.numel == 0 || g.out_numel == 0) return ZT_OK;
    // T <= 4, r <= 2: the one-march kernel (g4_fused.hip)
    if (zt::guided4d_fused_supports(radius, g)) {
        bool contiguous = dtype_in == zt::kF32;
        int64_t st = 1;
        for (int d = 3; d >= 0; --d) {
            if (in_strides[d] != st) contiguous = false;
            st *= shape[d];
        }
        const float* v = static_cast<const float*>(in);
        if (!contiguous) {  // f32 C-order copy of the block in scratch
            if (int rc = ctx->ensure_scratch(sizeof(float) * (size_t)g.numel)) return rc;
            float* vv = static_cast<float*>(ctx->scratch);
            const size_t esz = zt::dtype_size(dtype_in);
            for (int64_t t = 0; t < shape[0]; ++t) {
                hipError_t e = zt::launch_cast_to_f32_3d(
                    static_cast<const char*>(in) + esz * t * in_strides[0], dtype_in, in_strides[1],
                    in_strides[2], vv + t * shape[1] * shape[2] * shape[3], shape[1], shape[2],
                    shape[3], ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "guided filter 4-D input cast");
            }
            v = vv;
        }
        if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
        hipError_t e = zt::launch_guided4d_fused(v, out, dtype_out, g, radius, eps, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "guided filter 4-D fused launch");
        if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
        return ZT_OK;
    }
    if (int rc = ctx->ensure_scratch((size_t)zt::guided4d_scratch_bytes(g.numel, true))) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_guided4d(in, dtype_in, out, dtype_out, g, radius, eps,
                                       ctx->scratch, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "guided filter 4-D launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

}  // namespace

namespace zt {
// Used by the host store / pipeline code (host/*.cpp) to report errors through zt_last_error().
int set_last_error(int code, const char* msg) {
    g_last_error = msg ? msg : "";
    return code;
}
}  // namespace zt

extern "C" {

int zt_abi_version(void) { return ZT_ABI_VERSION; }

const char* zt_last_error(void) { return g_last_error.c_str(); }

size_t zt_dtype_size(int dtype) { return zt::dtype_size(dtype); }

int zt_device_count(int* count) {
    if (!count) return fail(ZT_ERR_INVALID_PARAMETERS, "null count");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return ZT_OK;
}

int zt_ctx_create(int device, zt_ctx** out) {
    if (!out) return fail(ZT_ERR_INVALID_PARAMETERS, "null output pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return fail(ZT_ERR_DEVICE, "no HIP device available");
    }
    if (device < 0 || device >= n)
        return fail(ZT_ERR_INVALID_PARAMETERS, "device %d not in [0, %d)", device, n);
    ZT_HIP(hipSetDevice(device));
    zt_ctx* c = new zt_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming) != hipSuccess) {
        if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
        if (c->ev1) (void)hipEventDestroy(c->ev1);
        if (c->ev0) (void)hipEventDestroy(c->ev0);
        if (c->own) (void)hipStreamDestroy(c->own);
        delete c;
        return fail(ZT_ERR_DEVICE, "stream/event creation failed");
    }
    c->cur = c->own;
    c->timed = true;
    *out = c;
    return ZT_OK;
}

int zt_ctx_destroy(zt_ctx* ctx) {
    if (!ctx) return ZT_OK;
    DeviceGuard g(ctx->device);
    (void)hipStreamSynchronize(ctx->cur);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_switch) (void)hipEventDestroy(ctx->ev_switch);
    if (ctx->own) (void)hipStreamDestroy(ctx->own);
    delete ctx;
    return ZT_OK;
}

namespace {

// The context's one scratch buffer (and whatever else its calls share) is only safe while all of
// its work is ordered. A switch to a different stream therefore makes the new stream wait for an
// event recorded on the old one: everything issued from now on runs after everything issued so
// far. Setting the stream the context already has costs nothing, so a caller that sets the same
// stream before every call (default_context(), the device chains) issues no extra work. A stream
// that no entry point has used is left without a new record (a new context given its stream: the
// own stream then never receives a command), but the new stream still waits for the last record,
// so the order also holds across switches with no call between them (A -> B -> C: C waits for A).
int switch_stream(zt_ctx* ctx, hipStream_t s) {
    if (int rc = check_ctx(ctx)) return rc;
    if (s == ctx->cur) return ZT_OK;
    DeviceGuard g(ctx->device);
    if (ctx->issued) {
        const hipError_t e = hipEventRecord(ctx->ev_switch, ctx->cur);
        if (e == hipSuccess) {
            ctx->recorded = true;
        } else if (e == hipErrorInvalidHandle || e == hipErrorContextIsDestroyed) {
            // the caller has destroyed the stream being left, which it may only do once the work
            // on it is done (zarrs_tools_amd.h): nothing new is left to wait for
            (void)hipGetLastError();
        } else {
            return hip_fail(e, "hipEventRecord at a stream switch");
        }
    }
    if (ctx->recorded) ZT_HIP(hipStreamWaitEvent(s, ctx->ev_switch, 0));
    ctx->cur = s;
    ctx->issued = false;
    return ZT_OK;
}

}  // namespace

int zt_ctx_set_stream(zt_ctx* ctx, void* hip_stream) {
    // Used verbatim: NULL is the device's default (null) stream, which is what
    // torch.cuda.current_stream().cuda_stream returns for torch's default stream.
    return switch_stream(ctx, static_cast<hipStream_t>(hip_stream));
}

int zt_ctx_use_own_stream(zt_ctx* ctx) {
    return switch_stream(ctx, ctx ? ctx->own : nullptr);
}

int zt_ctx_get_stream(zt_ctx* ctx, void** hip_stream) {
    if (int rc = begin_call(ctx)) return rc;  // the caller may issue work on the stream it gets
    if (!hip_stream) return fail(ZT_ERR_INVALID_PARAMETERS, "null output pointer");
    *hip_stream = ctx->cur;
    return ZT_OK;
}

int zt_ctx_synchronize(zt_ctx* ctx) {
    if (int rc = check_ctx(ctx)) return rc;
    DeviceGuard g(ctx->device);
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    return ZT_OK;
}

int zt_ctx_scratch_bytes(zt_ctx* ctx, uint64_t* bytes) {
    if (int rc = check_ctx(ctx)) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null output pointer");
    *bytes = ctx->scratch_bytes;
    return ZT_OK;
}

int zt_ctx_release_scratch(zt_ctx* ctx) {
    if (int rc = check_ctx(ctx)) return rc;
    DeviceGuard g(ctx->device);
    if (ctx->scratch) {
        ZT_HIP(hipStreamSynchronize(ctx->cur));
        ZT_HIP(hipFree(ctx->scratch));
        ctx->scratch = nullptr;
        ctx->scratch_bytes = 0;
    }
    return ZT_OK;
}

int zt_ctx_last_kernel_ms(zt_ctx* ctx, float* ms) {
    if (int rc = check_ctx(ctx)) return rc;
    if (!ms) return fail(ZT_ERR_INVALID_PARAMETERS, "null output pointer");
    DeviceGuard g(ctx->device);
    ZT_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return ZT_OK;
}

// ---- guided filter ---------------------------------------------------------------------------

int zt_guided_filter_is_compatible(int dtype_in, int dtype_out) {
    // guided_filter.rs:208-224: every listed type is accepted for input and output.
    return dtypes_ok(dtype_in, dtype_out);
}

int zt_guided_filter_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                      int ndim, uint64_t* bytes) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null output pointer");
    // guided_filter.rs:234-237 (element sizes + num_elements * (f64 + 2 f32))
    uint64_t n = (uint64_t)numel(chunk_shape, ndim);
    *bytes = zt::dtype_size(dtype_in) + zt::dtype_size(dtype_out) + n * (8 + 4 * 2);
    return ZT_OK;
}

int zt_subset_overlap(const int64_t* array_shape, int ndim, const int64_t* subset_start,
                      const int64_t* subset_shape, const int64_t* overlap, int64_t* input_start,
                      int64_t* input_shape, int64_t* dst_in_src_start) {
    if (int rc = check_shape(array_shape, ndim, "array_shape")) return rc;
    if (!subset_start || !subset_shape || !overlap || !input_start || !input_shape ||
        !dst_in_src_start)
        return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer argument");
    for (int d = 0; d < ndim; ++d) {
        if (overlap[d] < 0 || subset_start[d] < 0 || subset_shape[d] < 0 ||
            subset_start[d] + subset_shape[d] > array_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "subset outside the array on axis %d", d);
        // array_subset_overlap.rs:12-29
        int64_t s = subset_start[d] > overlap[d] ? subset_start[d] - overlap[d] : 0;
        int64_t e = std::min(subset_start[d] + subset_shape[d] + overlap[d], array_shape[d]);
        input_start[d] = s;
        input_shape[d] = e - s;
        dst_in_src_start[d] = subset_start[d] - s;
    }
    return ZT_OK;
}

int zt_guided_filter_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                   const int64_t* in_shape, const int64_t* in_strides, int ndim,
                                   const int64_t* out_start, const int64_t* out_shape,
                                   int dtype_out, void* out, const int64_t* out_strides,
                                   float epsilon, int radius) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = radius_ok(radius)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (!out_start || !out_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null output region");
    for (int d = 0; d < ndim; ++d)
        if (out_start[d] < 0 || out_shape[d] < 0 || out_start[d] + out_shape[d] > in_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "output region outside the block on axis %d",
                        d);
    if (numel(out_shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    int64_t is[ZT_MAX_DIMS], os[ZT_MAX_DIMS];
    if (in_strides) std::copy(in_strides, in_strides + ndim, is);
    else c_strides(in_shape, ndim, is);
    if (out_strides) std::copy(out_strides, out_strides + ndim, os);
    else c_strides(out_shape, ndim, os);
    DeviceGuard g(ctx->device);
    if (ndim <= 3 && zt::fused_supports_radius(radius) && is[ndim - 1] == 1 &&
        os[ndim - 1] == 1) {
        int64_t dom[3] = {1, 1, 1}, ost[3] = {0, 0, 0}, osh[3] = {1, 1, 1};
        int64_t isz = 0, isy = 0, osz = 0, osy = 0;
        for (int d = 0; d < ndim; ++d) {
            dom[3 - ndim + d] = in_shape[d];
            ost[3 - ndim + d] = out_start[d];
            osh[3 - ndim + d] = out_shape[d];
        }
        if (ndim == 3) { isz = is[0]; isy = is[1]; osz = os[0]; osy = os[1]; }
        if (ndim == 2) { isy = is[0]; osy = os[0]; }
        if (ndim == 1) { isy = dom[2]; osy = osh[2]; }
        if (fused_planes_fit(dom, isy, osh, osy, dtype_in, dtype_out))
            return run_fused3(ctx, dtype_in, in, dom, 0, dom[0], isz, isy, ost, osh, dtype_out,
                              out, osz, osy, epsilon, radius, 0);
    }
    if (use_guided4d(ndim, radius, is, in_shape))
        return run_guided4d(ctx, dtype_in, in, in_shape, is, out_start, out_shape, dtype_out, out,
                            os, epsilon, radius);
    return run_separable(ctx, dtype_in, in, in_shape, is, ndim, out_start, out_shape, dtype_out,
                         out, os, epsilon, radius);
}

int zt_guided_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                 void* out, const int64_t* shape, int ndim,
                                 const int64_t* chunk_shape, float epsilon, int radius,
                                 const int64_t* chunk_grid_start,
                                 const int64_t* chunk_grid_count) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = radius_ok(radius)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!chunk_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null chunk_shape");
    int64_t grid[ZT_MAX_DIMS], g0[ZT_MAX_DIMS], gn[ZT_MAX_DIMS];
    for (int d = 0; d < ndim; ++d) {
        if (chunk_shape[d] <= 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk extent must be positive");
        grid[d] = (shape[d] + chunk_shape[d] - 1) / chunk_shape[d];
        g0[d] = chunk_grid_start ? chunk_grid_start[d] : 0;
        gn[d] = chunk_grid_count ? chunk_grid_count[d] : grid[d];
        if (g0[d] < 0 || gn[d] < 0 || g0[d] + gn[d] > grid[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk grid range outside the grid on axis %d",
                        d);
    }
    if (numel(gn, ndim) == 0 || numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    // Output region = the box of chunks (chunk_subset_bounded per chunk, guided_filter.rs:87).
    int64_t ostart[ZT_MAX_DIMS], oshape[ZT_MAX_DIMS], strides[ZT_MAX_DIMS];
    for (int d = 0; d < ndim; ++d) {
        ostart[d] = g0[d] * chunk_shape[d];
        oshape[d] = std::min((g0[d] + gn[d]) * chunk_shape[d], shape[d]) - ostart[d];
    }
    c_strides(shape, ndim, strides);
    DeviceGuard g(ctx->device);
    const size_t esz_in = zt::dtype_size(dtype_in), esz_out = zt::dtype_size(dtype_out);
    int64_t fdom[3] = {1, 1, 1}, fosh[3] = {1, 1, 1};
    for (int d = 0; d < ndim && ndim <= 3; ++d) {
        fdom[3 - ndim + d] = shape[d];
        fosh[3 - ndim + d] = oshape[d];
    }
    if (ndim <= 3 && zt::fused_supports_radius(radius) &&
        fused_planes_fit(fdom, fdom[2], fosh, fdom[2], dtype_in, dtype_out)) {
        // One launch for the whole box: every window clamps at the array bounds, which is what
        // the reference's per-chunk 2r halo (clamped to the array) produces.
        int64_t dom[3] = {1, 1, 1}, ost[3] = {0, 0, 0}, osh[3] = {1, 1, 1};
        for (int d = 0; d < ndim; ++d) {
            dom[3 - ndim + d] = shape[d];
            ost[3 - ndim + d] = ostart[d];
            osh[3 - ndim + d] = oshape[d];
        }
        int64_t sz = ndim == 3 ? strides[0] : 0, sy = ndim >= 2 ? strides[ndim - 2] : 0;
        char* obase = static_cast<char*>(out) +
                      esz_out * (ost[0] * (ndim == 3 ? sz : 0) + ost[1] * sy + ost[2]);
        (void)esz_in;
        int chunk_depth = ndim == 3 ? (int)chunk_shape[0] : 0;
        return run_fused3(ctx, dtype_in, in, dom, 0, dom[0], sz, sy, ost, osh, dtype_out, obase,
                          sz, sy, epsilon, radius, chunk_depth > 0 ? chunk_depth : 1);
    }
    int64_t ov[ZT_MAX_DIMS];
    for (int d = 0; d < ndim; ++d) ov[d] = (int64_t)((radius * 2) & 0xFF);
    // Separable / four-kernel 4-D paths: as few launches as the scratch allows. Chunks are
    // grouped along the trailing axes — the whole box when its scratch (plus its 2r halo) fits
    // in half the free device memory, else rows of chunks over axes k..ndim-1 for the smallest k
    // that fits, down to single chunks. Chunked == whole with the halo; rows
    // spare the per-chunk halo recompute of the grouped axes and the launches' tails.
    size_t free_b = 0, total_b = 0;
    const bool have_info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    (void)hipGetLastError();
    auto need_of = [&](const int64_t* ish) -> size_t {
        return use_guided4d(ndim, radius, strides, ish)
                   ? (size_t)zt::guided4d_scratch_bytes(numel(ish, ndim), true)
                   : sizeof(float) * (size_t)zt::separable_scratch_floats(numel(ish, ndim));
    };
    // ZT_SCRATCH_LIMIT (bytes, tests): a smaller budget, to exercise the row / chunk grouping
    const char* lim_env = getenv("ZT_SCRATCH_LIMIT");
    const size_t lim = lim_env ? (size_t)strtoull(lim_env, nullptr, 10) : SIZE_MAX;
    auto fits = [&](size_t need) {
        if (need > lim) return false;
        return ctx->scratch_bytes >= need ||
               (have_info && need + ctx->scratch_bytes <= free_b / 2);
    };
    // k = number of leading axes iterated chunk by chunk (0: the whole box in one call). A
    // group's input is at most one chunk plus its two halos along axes < k and the box (plus
    // its halos) along the rest; the budget check uses that largest group.
    int64_t bis0[ZT_MAX_DIMS], bish[ZT_MAX_DIMS], bdst[ZT_MAX_DIMS];
    if (int rc = zt_subset_overlap(shape, ndim, ostart, oshape, ov, bis0, bish, bdst)) return rc;
    int k = 0;
    for (; k < ndim; ++k) {
        int64_t ish[ZT_MAX_DIMS];
        for (int d = 0; d < ndim; ++d)
            ish[d] = d < k ? std::min(chunk_shape[d] + 2 * ov[d], bish[d]) : bish[d];
        if (fits(need_of(ish))) break;
    }
    // iterate the chunk grid of axes < k; each call covers those chunks' full extent along >= k
    int64_t ngroups = 1;
    for (int d = 0; d < k; ++d) ngroups *= gn[d];
    for (int64_t c = 0; c < ngroups; ++c) {
        int64_t rem = c, cs[ZT_MAX_DIMS], csh[ZT_MAX_DIMS];
        for (int d = ndim - 1; d >= 0; --d) {
            if (d >= k) {
                cs[d] = ostart[d];
                csh[d] = oshape[d];
                continue;
            }
            int64_t ci = g0[d] + rem % gn[d];
            rem /= gn[d];
            cs[d] = ci * chunk_shape[d];
            csh[d] = std::min(cs[d] + chunk_shape[d], shape[d]) - cs[d];
        }
        int64_t is0[ZT_MAX_DIMS], ish[ZT_MAX_DIMS], dst[ZT_MAX_DIMS];
        int rc = zt_subset_overlap(shape, ndim, cs, csh, ov, is0, ish, dst);
        if (rc) return rc;
        int64_t ioff = 0, ooff = 0;
        for (int d = 0; d < ndim; ++d) {
            ioff += is0[d] * strides[d];
            ooff += cs[d] * strides[d];
        }
        rc = use_guided4d(ndim, radius, strides, ish)
                 ? run_guided4d(ctx, dtype_in, static_cast<const char*>(in) + esz_in * ioff, ish,
                                strides, dst, csh, dtype_out,
                                static_cast<char*>(out) + esz_out * ooff, strides, epsilon,
                                radius)
                 : run_separable(ctx, dtype_in, static_cast<const char*>(in) + esz_in * ioff, ish,
                                 strides, ndim, dst, csh, dtype_out,
                                 static_cast<char*>(out) + esz_out * ooff, strides, epsilon,
                                 radius);
        if (rc) return rc;
    }
    return ZT_OK;
}

int zt_guided_filter_apply_slab(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                void* out, const int64_t* global_shape, int64_t in_z0,
                                int64_t in_nz, int64_t out_z0, int64_t out_nz,
                                const int64_t* chunk_shape, float epsilon, int radius) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = radius_ok(radius)) return rc;
    if (int rc = check_shape(global_shape, 3, "global_shape")) return rc;
    if (!zt::fused_supports_radius(radius))
        return fail(ZT_ERR_INVALID_PARAMETERS, "slab form supports radius <= %d",
                    zt::kFusedMaxRadius);
    const int R = radius;
    if (in_z0 < 0 || in_nz < 0 || in_z0 + in_nz > global_shape[0] || out_z0 < in_z0 ||
        out_z0 + out_nz > in_z0 + in_nz)
        return fail(ZT_ERR_INVALID_PARAMETERS, "slab rows outside the array / input slab");
    // the slab must carry the 2r halo or reach the array edge
    if ((out_z0 - 2 * R < in_z0 && in_z0 > 0) ||
        (out_z0 + out_nz + 2 * R > in_z0 + in_nz && in_z0 + in_nz < global_shape[0]))
        return fail(ZT_ERR_INVALID_PARAMETERS, "input slab lacks the 2*radius halo rows");
    if (out_nz == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    const int64_t sy = global_shape[2], sz = global_shape[1] * global_shape[2];
    int64_t dom[3] = {global_shape[0], global_shape[1], global_shape[2]};
    int64_t ost[3] = {out_z0, 0, 0}, osh[3] = {out_nz, global_shape[1], global_shape[2]};
    if (!fused_planes_fit(dom, sy, osh, sy, dtype_in, dtype_out)) {
        // planes of >= 2 GiB: the separable path on the slab block (it carries the 2r halo, so
        // windows clamped at the block equal windows clamped at the array)
        const int64_t bsh[3] = {in_nz, global_shape[1], global_shape[2]};
        const int64_t bst[3] = {sz, sy, 1};
        const int64_t bos[3] = {out_z0 - in_z0, 0, 0};
        return run_separable(ctx, dtype_in, in, bsh, bst, 3, bos, osh, dtype_out, out, bst,
                             epsilon, radius);
    }
    int depth = chunk_shape && chunk_shape[0] > 0 ? (int)chunk_shape[0] : (int)out_nz;
    return run_fused3(ctx, dtype_in, in, dom, in_z0, in_nz, sz, sy, ost, osh, dtype_out, out, sz,
                      sy, epsilon, radius, depth);
}

// ---- Gaussian (gaussian.rs) -------------------------------------------------------------------

namespace {

// create_sampled_gaussian_kernel (gaussian.rs:252-267), operation for operation: t = sigma^2,
// scale = 1 / sqrt(2 * PI * t), tap(n) = scale * exp(-((n*n) as f32) / (2 * t)) with the
// platform libm expf (as the reference's f32::exp on Linux); taps = tap(half..1), tap(0..half).
int64_t gaussian_taps(float sigma, int64_t half, float* taps) {
    if (sigma == 0.0f) {
        if (taps) taps[0] = 1.0f;
        return 1;
    }
    if (taps) {
        const float pi = 3.14159265358979323846f;  // std::f32::consts::PI
        const float t = sigma * sigma;
        const float scale = 1.0f / sqrtf(2.0f * pi * t);
        for (int64_t n = 0; n <= half; ++n) {
            const float e = scale * expf(-((float)(uint64_t)(n * n) / (2.0f * t)));
            taps[half - n] = e;
            taps[half + n] = e;
        }
    }
    return 2 * half + 1;
}

int gaussian_args_ok(const float* sigma, const int64_t* half, int ndim) {
    if (!sigma || !half) return fail(ZT_ERR_INVALID_PARAMETERS, "null sigma / kernel_half_size");
    for (int d = 0; d < ndim; ++d) {
        if (half[d] < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative kernel_half_size");
        if (gaussian_taps(sigma[d], half[d], nullptr) > zt::kGaussMaxTaps)
            return fail(ZT_ERR_INVALID_PARAMETERS, "kernel_half_size %lld on axis %d exceeds %d",
                        (long long)half[d], d, (zt::kGaussMaxTaps - 1) / 2);
    }
    return ZT_OK;
}

// Gaussian::apply_ndarray on a C-order block, writing only the output region: one pass per
// axis (gaussian.hip), each restricted to what the later passes read, through two f32 scratch
// buffers; the last pass writes f32 outputs in place, other types through a cast.
int run_gaussian(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape, int ndim,
                 const int64_t* out_start, const int64_t* out_shape, int dtype_out, void* out,
                 const float* sigma, const int64_t* half) {
    const int64_t nout = numel(out_shape, ndim);
    if (nout == 0) return ZT_OK;
    int64_t cur[ZT_MAX_DIMS];
    std::copy(in_shape, in_shape + ndim, cur);
    int64_t maxn = 0;
    for (int d = 0; d < ndim; ++d) {
        cur[d] = out_shape[d];
        maxn = std::max(maxn, numel(cur, ndim));
    }
    const bool cast_out = dtype_out != zt::kF32;
    if (int rc = ctx->ensure_scratch(sizeof(float) * 2 * (size_t)maxn)) return rc;
    float* bufs[2] = {static_cast<float*>(ctx->scratch), static_cast<float*>(ctx->scratch) + maxn};
    std::copy(in_shape, in_shape + ndim, cur);
    const void* src = in;
    int sdt = dtype_in;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    // the last three axes in one z-march when they share one tap vector length that fits it
    if (ndim >= 3) {
        zt::GaussZYX pz{};
        pz.outer = numel(in_shape, ndim - 3);
        float w[zt::kGaussMaxTaps];
        bool same = true;
        for (int a = 0; a < 3; ++a) {
            const int d = ndim - 3 + a;
            const int64_t len = gaussian_taps(sigma[d], half[d], w);
            if (a == 0) pz.len = (int)len;
            if (len != pz.len || len > zt::kGaussZYXMaxLen) {
                same = false;
                break;
            }
            std::copy(w, w + len, pz.w[a]);
            pz.n[a] = in_shape[d];
            pz.on[a] = out_shape[d];
            pz.o0[a] = out_start[d];
        }
        if (same && zt::gaussian_zyx_supported(pz, dtype_in)) {
            // earlier axes (ndim > 3) first, pass by pass, then the fused three
            for (int d = 0; d < ndim - 3; ++d) {
                zt::GaussPass p{};
                p.outer = numel(cur, d);
                p.n = cur[d];
                p.on = out_shape[d];
                p.o0 = out_start[d];
                p.inner = numel(cur + d + 1, ndim - d - 1);
                p.len = (int)gaussian_taps(sigma[d], half[d], p.w);
                p.mid = p.len / 2;
                float* dst = bufs[d & 1];
                hipError_t e = zt::launch_gaussian_pass(src, sdt, dst, p, ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "gaussian pass launch");
                src = dst;
                sdt = zt::kF32;
                cur[d] = out_shape[d];
            }
            pz.outer = numel(cur, ndim - 3);
            float* dst = !cast_out ? static_cast<float*>(out) : bufs[(ndim - 3) & 1];
            hipError_t e = zt::launch_gaussian_zyx(src, sdt, dst, pz, ctx->cur);
            if (e != hipSuccess) return hip_fail(e, "gaussian z/y/x march launch");
            if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
            if (cast_out) {
                e = zt::launch_cast_from_f32_3d(dst, dtype_out, out, 0, 0, 1, 1, nout, ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "gaussian output cast");
            }
            return ZT_OK;
        }
    }
    // the last two axes in one fused pass when their kernels fit it (and the y extent fits a grid)
    const bool fuse_yx = ndim >= 2 &&
                         gaussian_taps(sigma[ndim - 2], half[ndim - 2], nullptr) <=
                             zt::kGaussYXMaxLen &&
                         gaussian_taps(sigma[ndim - 1], half[ndim - 1], nullptr) <=
                             zt::kGaussYXMaxLen &&
                         (out_shape[ndim - 2] + 31) / 32 <= 65535;
    const int nsep = fuse_yx ? ndim - 2 : ndim;
    for (int d = 0; d < nsep; ++d) {
        zt::GaussPass p{};
        p.outer = numel(cur, d);
        p.n = cur[d];
        p.on = out_shape[d];
        p.o0 = out_start[d];
        p.inner = numel(cur + d + 1, ndim - d - 1);
        p.len = (int)gaussian_taps(sigma[d], half[d], p.w);
        p.mid = p.len / 2;
        float* dst = (d == ndim - 1 && !cast_out) ? static_cast<float*>(out) : bufs[d & 1];
        hipError_t e = zt::launch_gaussian_pass(src, sdt, dst, p, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "gaussian pass launch");
        src = dst;
        sdt = zt::kF32;
        cur[d] = out_shape[d];
    }
    if (fuse_yx) {
        const int dy = ndim - 2, dx = ndim - 1;
        zt::GaussPass py{}, px{};
        py.n = cur[dy];
        py.on = out_shape[dy];
        py.o0 = out_start[dy];
        py.len = (int)gaussian_taps(sigma[dy], half[dy], py.w);
        py.mid = py.len / 2;
        px.n = cur[dx];
        px.on = out_shape[dx];
        px.o0 = out_start[dx];
        px.len = (int)gaussian_taps(sigma[dx], half[dx], px.w);
        px.mid = px.len / 2;
        float* dst = !cast_out ? static_cast<float*>(out) : bufs[nsep & 1];
        hipError_t e = zt::launch_gaussian_yx(src, sdt, dst, numel(cur, dy), py, px, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "gaussian y/x pass launch");
        src = dst;
    }
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (cast_out) {
        hipError_t e = zt::launch_cast_from_f32_3d(static_cast<const float*>(src), dtype_out, out,
                                                   0, 0, 1, 1, nout, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "gaussian output cast");
    }
    return ZT_OK;
}

}  // namespace

int zt_gaussian_kernel(float sigma, int64_t kernel_half_size, float* taps, int64_t* len) {
    if (!len || kernel_half_size < 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "null len or negative kernel_half_size");
    *len = gaussian_taps(sigma, kernel_half_size, taps);
    return ZT_OK;
}

int zt_gaussian_is_compatible(int dtype_in, int dtype_out) {
    // gaussian.rs:123-147: every listed type is accepted for input and output.
    return dtypes_ok(dtype_in, dtype_out);
}

int zt_gaussian_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                 int ndim, const int64_t* kernel_half_size, uint64_t* bytes) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes || !kernel_half_size) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    // gaussian.rs:149-168
    uint64_t nin = 1;
    for (int d = 0; d < ndim; ++d) nin *= (uint64_t)(chunk_shape[d] + 2 * kernel_half_size[d]);
    const uint64_t nout = (uint64_t)numel(chunk_shape, ndim);
    *bytes = nin * (zt::dtype_size(dtype_in) + 4 * 2) + nout * (4 + zt::dtype_size(dtype_out));
    return ZT_OK;
}

int zt_gaussian_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape,
                              int ndim, const int64_t* out_start, const int64_t* out_shape,
                              int dtype_out, void* out, const float* sigma,
                              const int64_t* kernel_half_size) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (int rc = gaussian_args_ok(sigma, kernel_half_size, ndim)) return rc;
    if (!out_start || !out_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null output region");
    for (int d = 0; d < ndim; ++d)
        if (out_start[d] < 0 || out_shape[d] < 0 || out_start[d] + out_shape[d] > in_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "output region outside the block on axis %d",
                        d);
    if (numel(out_shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    return run_gaussian(ctx, dtype_in, in, in_shape, ndim, out_start, out_shape, dtype_out, out,
                        sigma, kernel_half_size);
}

int zt_gaussian_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out, void* out,
                            const int64_t* shape, int ndim, const int64_t* chunk_shape,
                            const float* sigma, const int64_t* kernel_half_size) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (int rc = gaussian_args_ok(sigma, kernel_half_size, ndim)) return rc;
    if (!chunk_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null chunk_shape");
    for (int d = 0; d < ndim; ++d)
        if (chunk_shape[d] <= 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk extent must be positive");
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    // Every chunk with its kernel_half_size halo (clamped to the array) equals the whole array
    // with replicate edges at the array bounds: the taps' mid is the halo, so a window clamps
    // inside a chunk's block only where it clamps at the array.
    int64_t zero[ZT_MAX_DIMS] = {0};
    DeviceGuard g(ctx->device);
    return run_gaussian(ctx, dtype_in, in, shape, ndim, zero, shape, dtype_out, out, sigma,
                        kernel_half_size);
}

// ---- gradient magnitude (gradient_magnitude.rs) ---------------------------------------------------

namespace {

// GradientMagnitude::apply_ndarray on a C-order block, writing only the output region.
int run_gradient_magnitude(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape,
                           int ndim, const int64_t* out_start, const int64_t* out_shape,
                           int dtype_out, void* out, int op) {
    const int64_t nout = numel(out_shape, ndim), nin = numel(in_shape, ndim);
    if (nout == 0) return ZT_OK;
    // 3-D Sobel: the fused z-march (f32 region; other output types through a cast)
    if (ndim == 3 && op == ZT_GM_SOBEL) {
        zt::GMSobel3 p{};
        for (int d = 0; d < 3; ++d) {
            p.n[d] = in_shape[d];
            p.on[d] = out_shape[d];
            p.o0[d] = out_start[d];
        }
        if (zt::gm_sobel3_supported(p)) {
            const bool cast_out = dtype_out != zt::kF32;
            if (cast_out)
                if (int rc = ctx->ensure_scratch(sizeof(float) * (size_t)nout)) return rc;
            float* dst = cast_out ? static_cast<float*>(ctx->scratch) : static_cast<float*>(out);
            if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
            hipError_t e = zt::launch_gm_sobel3(in, dtype_in, dst, p, ctx->cur);
            if (e != hipSuccess) return hip_fail(e, "gradient magnitude z/y/x march launch");
            if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
            if (cast_out) {
                e = zt::launch_cast_from_f32_3d(dst, dtype_out, out, 0, 0, 1, 1, nout, ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "gradient magnitude output cast");
            }
            return ZT_OK;
        }
    }
    // the reference's passes on the whole block: staging_in / staging_out / gradient_magnitude
    if (int rc = ctx->ensure_scratch(sizeof(float) * 3 * (size_t)nin)) return rc;
    float* sa = static_cast<float*>(ctx->scratch);
    float* sb = sa + nin;
    float* g = sb + nin;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    for (int axis = 0; axis < ndim; ++axis) {
        const float* s = nullptr;
        if (op == ZT_GM_SOBEL) {
            const void* src = in;
            int sdt = dtype_in;
            for (int i = 0; i < ndim; ++i) {
                float* dst = (i & 1) ? sb : sa;
                hipError_t e = zt::launch_gm_pass(src, sdt, dst, numel(in_shape, i), in_shape[i],
                                                  numel(in_shape + i + 1, ndim - i - 1),
                                                  i == axis, ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "gradient magnitude pass launch");
                src = dst;
                sdt = zt::kF32;
            }
            s = static_cast<const float*>(src);
        } else {
            hipError_t e = zt::launch_gm_pass(in, dtype_in, sa, numel(in_shape, axis),
                                              in_shape[axis],
                                              numel(in_shape + axis + 1, ndim - axis - 1), true,
                                              ctx->cur);
            if (e != hipSuccess) return hip_fail(e, "gradient magnitude pass launch");
            s = sa;
        }
        hipError_t e = zt::launch_gm_accumulate(g, s, nin, axis == 0, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "gradient magnitude accumulate launch");
    }
    zt::NdGeom geom{};
    geom.ndim = ndim;
    geom.numel = nin;
    geom.out_numel = nout;
    for (int d = 0; d < ndim; ++d) {
        geom.shape[d] = in_shape[d];
        geom.out_start[d] = out_start[d];
        geom.out_shape[d] = out_shape[d];
    }
    hipError_t e = zt::launch_gm_finish(g, dtype_out, out, geom, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "gradient magnitude finish launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int gm_op_ok(int op) {
    if (op != ZT_GM_SOBEL && op != ZT_GM_CENTRAL_DIFFERENCE)
        return fail(ZT_ERR_INVALID_PARAMETERS, "unknown gradient magnitude operator %d", op);
    return ZT_OK;
}

}  // namespace

int zt_gradient_magnitude_is_compatible(int dtype_in, int dtype_out) {
    // gradient_magnitude.rs:151-175: every listed type is accepted for input and output.
    return dtypes_ok(dtype_in, dtype_out);
}

int zt_gradient_magnitude_memory_per_chunk(int dtype_in, int dtype_out,
                                           const int64_t* chunk_shape, int ndim,
                                           uint64_t* bytes) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    // gradient_magnitude.rs:177-195
    uint64_t nin = 1;
    for (int d = 0; d < ndim; ++d) nin *= (uint64_t)(chunk_shape[d] + 2);
    const uint64_t nout = (uint64_t)numel(chunk_shape, ndim);
    *bytes = nin * (zt::dtype_size(dtype_in) + 4 * 4) + nout * (4 + zt::dtype_size(dtype_out));
    return ZT_OK;
}

int zt_gradient_magnitude_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                        const int64_t* in_shape, int ndim,
                                        const int64_t* out_start, const int64_t* out_shape,
                                        int dtype_out, void* out, int op) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (int rc = gm_op_ok(op)) return rc;
    if (!out_start || !out_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null output region");
    for (int d = 0; d < ndim; ++d)
        if (out_start[d] < 0 || out_shape[d] < 0 || out_start[d] + out_shape[d] > in_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "output region outside the block on axis %d",
                        d);
    if (numel(out_shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    return run_gradient_magnitude(ctx, dtype_in, in, in_shape, ndim, out_start, out_shape,
                                  dtype_out, out, op);
}

int zt_gradient_magnitude_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                      void* out, const int64_t* shape, int ndim,
                                      const int64_t* chunk_shape, int op) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (int rc = gm_op_ok(op)) return rc;
    if (!chunk_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null chunk_shape");
    for (int d = 0; d < ndim; ++d)
        if (chunk_shape[d] <= 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk extent must be positive");
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    // Every chunk with its halo of 1 (clamped to the array) equals the whole array with
    // replicate edges at the array bounds: each pass reaches 1, so an index clamps inside a
    // chunk's block only where it clamps at the array (as for the Gaussian above).
    int64_t zero[ZT_MAX_DIMS] = {0};
    DeviceGuard g(ctx->device);
    return run_gradient_magnitude(ctx, dtype_in, in, shape, ndim, zero, shape, dtype_out, out,
                                  op);
}

// ---- rank filters: minimum, median, maximum (rank.hip; no counterpart in the reference) ----------

namespace {

int rank_args_ok(int kind, const int64_t* half, int ndim) {
    if (kind != ZT_RANK_MINIMUM && kind != ZT_RANK_MEDIAN && kind != ZT_RANK_MAXIMUM)
        return fail(ZT_ERR_INVALID_PARAMETERS, "unknown rank filter kind %d", kind);
    if (!half) return fail(ZT_ERR_INVALID_PARAMETERS, "null kernel_half_size");
    int64_t window = 1;
    for (int d = 0; d < ndim; ++d) {
        if (half[d] < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative kernel_half_size");
        if (half[d] > (int64_t)1 << 30)
            return fail(ZT_ERR_INVALID_PARAMETERS, "kernel_half_size %lld on axis %d is too large",
                        (long long)half[d], d);
        if (kind == ZT_RANK_MEDIAN) {
            window *= 2 * half[d] + 1;  // <= 4096 * (2^31 + 1) before the check: no overflow
            if (window > zt::kRankMedianMaxWindow)
                return fail(ZT_ERR_INVALID_PARAMETERS,
                            "median window of more than %lld elements",
                            (long long)zt::kRankMedianMaxWindow);
        }
    }
    return ZT_OK;
}

size_t rank_align(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// The filter on a C-order block, writing only the output region: the selection in the input
// type (into `out`, or into scratch when the output type differs), then the `as` cast.
int run_rank_filter(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape, int ndim,
                    const int64_t* out_start, const int64_t* out_shape, int dtype_out, void* out,
                    int kind, const int64_t* half) {
    const int64_t nout = numel(out_shape, ndim);
    if (nout == 0) return ZT_OK;
    const size_t esz = zt::dtype_size(dtype_in);
    const int mode = zt::rank_key_mode(dtype_in);
    const bool cast_out = dtype_out != dtype_in;
    const size_t sel_bytes = cast_out ? rank_align((size_t)nout * esz) : 0;
    bool fused = ndim == 3 && half[0] == 1 && half[1] == 1 && half[2] == 1;
    zt::Rank3 p3{};
    if (fused) {
        for (int d = 0; d < 3; ++d) {
            p3.n[d] = in_shape[d];
            p3.on[d] = out_shape[d];
            p3.o0[d] = out_start[d];
        }
        fused = zt::rank3_supported(p3, (int)esz);
    }
    // minimum / maximum pass by pass: every axis with a window or a cropped extent
    int axes[ZT_MAX_DIMS], naxes = 0;
    int64_t maxn = 0;
    if (!fused && kind != ZT_RANK_MEDIAN) {
        int64_t cur[ZT_MAX_DIMS];
        std::copy(in_shape, in_shape + ndim, cur);
        for (int d = 0; d < ndim; ++d) {
            if (half[d] == 0 && out_shape[d] == in_shape[d]) continue;
            cur[d] = out_shape[d];
            axes[naxes++] = d;
            maxn = std::max(maxn, numel(cur, ndim));
        }
    }
    const size_t buf_bytes = naxes > 1 ? rank_align((size_t)maxn * esz) : 0;
    if (sel_bytes + 2 * buf_bytes > 0)
        if (int rc = ctx->ensure_scratch(sel_bytes + 2 * buf_bytes)) return rc;
    char* base = static_cast<char*>(ctx->scratch);
    void* sel = cast_out ? static_cast<void*>(base) : out;  // the selected region, input type
    void* bufs[2] = {base + sel_bytes, base + sel_bytes + buf_bytes};
    const void* res = sel;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    if (fused) {
        hipError_t e = zt::launch_rank3(in, sel, (int)esz, mode, kind, p3, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "rank filter z/y/x march launch");
    } else if (kind == ZT_RANK_MEDIAN) {
        zt::RankMedian pm{};
        pm.ndim = ndim;
        pm.out_numel = nout;
        int64_t window = 1;
        for (int d = 0; d < ndim; ++d) {
            pm.shape[d] = in_shape[d];
            pm.half[d] = half[d];
            pm.out_start[d] = out_start[d];
            pm.out_shape[d] = out_shape[d];
            window *= 2 * half[d] + 1;
        }
        c_strides(in_shape, ndim, pm.stride);
        pm.rows = (int)(window / (2 * half[ndim - 1] + 1));
        pm.rank = (int)((window - 1) / 2);
        hipError_t e = zt::launch_rank_median(in, sel, (int)esz, mode, pm, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "rank filter median launch");
    } else if (naxes == 0) {
        res = in;  // the identity on the whole block
        if (!cast_out) ZT_HIP(hipMemcpyAsync(out, in, (size_t)nout * esz, hipMemcpyDeviceToDevice,
                                             ctx->cur));
    } else {
        int64_t cur[ZT_MAX_DIMS];
        std::copy(in_shape, in_shape + ndim, cur);
        const void* src = in;
        for (int a = 0; a < naxes; ++a) {
            const int d = axes[a];
            zt::RankPass p{};
            p.outer = numel(cur, d);
            p.n = cur[d];
            p.on = out_shape[d];
            p.o0 = out_start[d];
            p.h = half[d];
            p.inner = numel(cur + d + 1, ndim - d - 1);
            void* dst = a == naxes - 1 ? sel : bufs[a & 1];
            hipError_t e = zt::launch_rank_pass(src, dst, (int)esz, mode, kind == ZT_RANK_MAXIMUM,
                                                p, ctx->cur);
            if (e != hipSuccess) return hip_fail(e, "rank filter pass launch");
            src = dst;
            cur[d] = out_shape[d];
        }
    }
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (cast_out) {
        hipError_t e = zt::launch_reencode_cast(res, dtype_in, out, dtype_out, nout, ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "rank filter output cast");
    }
    return ZT_OK;
}

}  // namespace

int zt_rank_filter_is_compatible(int dtype_in, int dtype_out) {
    // the selection is a matter of storage bits: all 13 types in, and out through the `as` cast
    return dtypes_ok(dtype_in, dtype_out);
}

int zt_rank_filter_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                    int ndim, const int64_t* kernel_half_size, uint64_t* bytes) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes || !kernel_half_size) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    for (int d = 0; d < ndim; ++d)
        if (kernel_half_size[d] < 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "negative kernel_half_size");
    // the input block, two pass buffers, and the selected block before the cast
    uint64_t nin = 1;
    for (int d = 0; d < ndim; ++d) nin *= (uint64_t)(chunk_shape[d] + 2 * kernel_half_size[d]);
    const uint64_t nout = (uint64_t)numel(chunk_shape, ndim);
    const uint64_t si = zt::dtype_size(dtype_in), so = zt::dtype_size(dtype_out);
    *bytes = nin * 3 * si + nout * (si + so);
    return ZT_OK;
}

int zt_rank_filter_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                 const int64_t* in_shape, int ndim, const int64_t* out_start,
                                 const int64_t* out_shape, int dtype_out, void* out, int kind,
                                 const int64_t* kernel_half_size) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (int rc = rank_args_ok(kind, kernel_half_size, ndim)) return rc;
    if (!out_start || !out_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null output region");
    for (int d = 0; d < ndim; ++d)
        if (out_start[d] < 0 || out_shape[d] < 0 || out_start[d] + out_shape[d] > in_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "output region outside the block on axis %d",
                        d);
    if (numel(out_shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (in == out) return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    DeviceGuard g(ctx->device);
    return run_rank_filter(ctx, dtype_in, in, in_shape, ndim, out_start, out_shape, dtype_out,
                           out, kind, kernel_half_size);
}

int zt_rank_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                               void* out, const int64_t* shape, int ndim,
                               const int64_t* chunk_shape, int kind,
                               const int64_t* kernel_half_size) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (int rc = rank_args_ok(kind, kernel_half_size, ndim)) return rc;
    if (!chunk_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null chunk_shape");
    for (int d = 0; d < ndim; ++d)
        if (chunk_shape[d] <= 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk extent must be positive");
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (in == out) return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    // Every chunk with its kernel_half_size halo (clamped to the array) equals the whole array
    // with replicate edges at the array bounds: a window index clamps inside a chunk's block only
    // where it clamps at the array (as for the Gaussian above).
    int64_t zero[ZT_MAX_DIMS] = {0};
    DeviceGuard g(ctx->device);
    return run_rank_filter(ctx, dtype_in, in, shape, ndim, zero, shape, dtype_out, out, kind,
                           kernel_half_size);
}

// ---- summed-area table (summed_area_table.rs) ------------------------------------------------

namespace {

// SummedAreaTable::apply on a C-order block: the scans run last axis to first; the first reads
// `in` (casting to dtype_out), the others work on `out` in place. `carry` seeds the axis-0 scan
// and receives its last plane.
int run_summed_area_table(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* shape,
                          int ndim, int dtype_out, void* out, void* carry) {
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    for (int axis = ndim - 1; axis >= 0; --axis) {
        const bool first = axis == ndim - 1;
        void* seed = axis == 0 ? carry : nullptr;
        hipError_t e = zt::launch_sat_pass(first ? in : out, first ? dtype_in : dtype_out, out,
                                           dtype_out, numel(shape, axis), shape[axis],
                                           numel(shape + axis + 1, ndim - axis - 1), seed, seed,
                                           ctx->cur);
        if (e != hipSuccess) return hip_fail(e, "summed area table pass launch");
    }
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

}  // namespace

int zt_summed_area_table_is_compatible(int dtype_in, int dtype_out) {
    // summed_area_table.rs:110-134: every listed type is accepted for input and output.
    return dtypes_ok(dtype_in, dtype_out);
}

int zt_summed_area_table_memory_per_chunk(int dtype_in, int dtype_out, const int64_t* chunk_shape,
                                          int ndim, uint64_t* bytes) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    // summed_area_table.rs:136-142 (sic): one element of each type, whatever the chunk shape
    *bytes = zt::dtype_size(dtype_in) + zt::dtype_size(dtype_out);
    return ZT_OK;
}

int zt_summed_area_table_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                       const int64_t* shape, int ndim, int dtype_out, void* out,
                                       void* carry) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (in == out) return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    DeviceGuard g(ctx->device);
    return run_summed_area_table(ctx, dtype_in, in, shape, ndim, dtype_out, out, carry);
}

int zt_summed_area_table_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                     void* out, const int64_t* shape, int ndim,
                                     const int64_t* chunk_shape) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!chunk_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null chunk_shape");
    for (int d = 0; d < ndim; ++d)
        if (chunk_shape[d] <= 0)
            return fail(ZT_ERR_INVALID_PARAMETERS, "chunk extent must be positive");
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (in == out) return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    // The reference carries each chunk's last plane into the next chunk along the scanned axis
    // (summed_area_table.rs:69, :94-97): the same left-to-right fold as one lane over the whole
    // axis, so the chunk grid does not enter the result.
    DeviceGuard g(ctx->device);
    return run_summed_area_table(ctx, dtype_in, in, shape, ndim, dtype_out, out, nullptr);
}

// ---- pointwise filters (reencode.rs, crop.rs, rescale.rs, clamp.rs, equal.rs, replace_value.rs) --

namespace {

// f64 `as` an integer type on the host: saturating, NaN -> 0 (clamp.rs:59-70's `min as TIn`)
extern "C++" {
template <typename T>
T sat_from_f64(double x) {
    if (!(x == x)) return (T)0;
    if (x <= (double)std::numeric_limits<T>::min()) return std::numeric_limits<T>::min();
    if (x >= (double)std::numeric_limits<T>::max()) return std::numeric_limits<T>::max();
    return (T)x;
}
}

// The class value (zt_kernels.hpp, PwClass) of the f64 `x as dtype`, as bits.
uint64_t class_bits_from_f64(double x, int dtype) {
    switch (dtype) {
    case ZT_BOOL: case ZT_UINT8: return sat_from_f64<uint8_t>(x);
    case ZT_UINT16: return sat_from_f64<uint16_t>(x);
    case ZT_UINT32: return sat_from_f64<uint32_t>(x);
    case ZT_UINT64: return sat_from_f64<uint64_t>(x);
    case ZT_INT8: return (uint32_t)(int32_t)sat_from_f64<int8_t>(x);
    case ZT_INT16: return (uint32_t)(int32_t)sat_from_f64<int16_t>(x);
    case ZT_INT32: return (uint32_t)sat_from_f64<int32_t>(x);
    case ZT_INT64: return (uint64_t)sat_from_f64<int64_t>(x);
    case ZT_BFLOAT16: return zt::f2u(zt::bf16_bits_to_f32(zt::f64_to_bf16_bits(x)));
    case ZT_FLOAT16: return zt::f2u(zt::f16_bits_to_f32(zt::f64_to_f16_bits(x)));
    case ZT_FLOAT32: return zt::f2u((float)x);
    default: return zt::d2u(x);
    }
}

// The class value of an element given as its storage bits (zero-extended little endian).
uint64_t class_bits_from_storage(uint64_t bits, int dtype) {
    switch (dtype) {
    case ZT_BOOL: case ZT_UINT8: return bits & 0xFFu;
    case ZT_UINT16: return bits & 0xFFFFu;
    case ZT_UINT32: return bits & 0xFFFFFFFFu;
    case ZT_INT8: return (uint32_t)(int32_t)(int8_t)bits;
    case ZT_INT16: return (uint32_t)(int32_t)(int16_t)bits;
    case ZT_INT32: return bits & 0xFFFFFFFFu;
    case ZT_BFLOAT16: return zt::f2u(zt::bf16_bits_to_f32((uint16_t)bits));
    case ZT_FLOAT16: return zt::f2u(zt::f16_bits_to_f32((uint16_t)bits));
    case ZT_FLOAT32: return bits & 0xFFFFFFFFu;
    default: return bits;  // int64, uint64, float64
    }
}

int pointwise_pair_ok(int kind, int dtype_in, int dtype_out) {
    if (kind < ZT_PW_REENCODE || kind > ZT_PW_REPLACE_VALUE)
        return fail(ZT_ERR_INVALID_PARAMETERS, "unknown pointwise op kind %d", kind);
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    // equal.rs:104-109: the output is bool or uint8
    if (kind == ZT_PW_EQUAL && dtype_out != ZT_BOOL && dtype_out != ZT_UINT8)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type %s (equal writes bool "
                    "or uint8)", dtype_name(dtype_out));
    return ZT_OK;
}

// Validate the type chain and translate the ABI ops to the kernel's program.
int build_pointwise_program(int dtype_in, const zt_pointwise_op* ops, int n_ops,
                            zt::PwProgram* prog) {
    if (!ops) return fail(ZT_ERR_INVALID_PARAMETERS, "null ops");
    if (n_ops < 1 || n_ops > ZT_PW_MAX_OPS)
        return fail(ZT_ERR_INVALID_PARAMETERS, "a pointwise program has 1 to %d ops, not %d",
                    ZT_PW_MAX_OPS, n_ops);
    std::memset(prog, 0, sizeof(*prog));
    prog->n_ops = n_ops;
    prog->dt_in = dtype_in;
    int dt = dtype_in;
    for (int k = 0; k < n_ops; ++k) {
        const zt_pointwise_op& o = ops[k];
        if (int rc = pointwise_pair_ok(o.kind, dt, o.dtype_out)) return rc;
        zt::PwOp& p = prog->ops[k];
        p.dt_out = o.dtype_out;
        switch (o.kind) {
        case ZT_PW_REENCODE: p.kind = zt::kPwCast; break;
        case ZT_PW_RESCALE:
            p.kind = zt::kPwRescale;
            p.flags = (o.flags & ZT_PW_ADD_FIRST) ? zt::kPwAddFirst : 0;
            p.a = o.imm0;
            p.b = o.imm1;
            break;
        case ZT_PW_CLAMP: {
            double lo, hi;
            std::memcpy(&lo, &o.imm0, 8);
            std::memcpy(&hi, &o.imm1, 8);
            p.kind = zt::kPwClamp;
            p.a = class_bits_from_f64(lo, dt);
            p.b = class_bits_from_f64(hi, dt);
            break;
        }
        case ZT_PW_EQUAL:
            p.kind = zt::kPwEqual;
            p.a = class_bits_from_storage(o.imm0, dt);
            break;
        default:
            p.kind = zt::kPwReplace;
            p.a = class_bits_from_storage(o.imm0, dt);
            p.b = class_bits_from_storage(o.imm1, o.dtype_out);
            break;
        }
        dt = o.dtype_out;
    }
    return ZT_OK;
}

}  // namespace

int zt_pointwise_is_compatible(int kind, int dtype_in, int dtype_out) {
    return pointwise_pair_ok(kind, dtype_in, dtype_out);
}

int zt_pointwise_memory_per_chunk(int kind, int dtype_in, int dtype_out,
                                  const int64_t* chunk_shape, int ndim, uint64_t* bytes) {
    if (int rc = pointwise_pair_ok(kind, dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    // reencode.rs:120-126, crop.rs:152-158: the output chunk; the others: input + output
    const uint64_t per = zt::dtype_size(dtype_out) +
                         (kind == ZT_PW_REENCODE ? 0 : zt::dtype_size(dtype_in));
    *bytes = (uint64_t)numel(chunk_shape, ndim) * per;
    return ZT_OK;
}

int zt_pointwise_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in, const int64_t* in_shape,
                               int ndim, const int64_t* sub_start, const int64_t* sub_shape,
                               const zt_pointwise_op* ops, int n_ops, void* out) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    zt::PwProgram prog;
    if (int rc = build_pointwise_program(dtype_in, ops, n_ops, &prog)) return rc;
    if ((sub_start == nullptr) != (sub_shape == nullptr))
        return fail(ZT_ERR_INVALID_PARAMETERS, "sub_start and sub_shape go together");
    int64_t start[ZT_MAX_DIMS], shape[ZT_MAX_DIMS], strides[ZT_MAX_DIMS];
    for (int d = 0; d < ndim; ++d) {
        start[d] = sub_start ? sub_start[d] : 0;
        shape[d] = sub_shape ? sub_shape[d] : in_shape[d];
        if (start[d] < 0 || shape[d] < 0 || start[d] + shape[d] > in_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "box outside the array on axis %d", d);
    }
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    const int64_t isz = (int64_t)zt::dtype_size(dtype_in);
    const int64_t osz = (int64_t)zt::dtype_size(prog.ops[n_ops - 1].dt_out);
    if (((uintptr_t)in % isz) != 0 || ((uintptr_t)out % osz) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    c_strides(in_shape, ndim, strides);
    // Merge axis d into axis d-1 where the box spans axis d (the pair is then one axis of the
    // source as well) and drop axes of extent 1: the whole contiguous array becomes one row.
    zt::PwGeom g{};
    int64_t ext[ZT_MAX_DIMS], str[ZT_MAX_DIMS];
    int n = 0;
    for (int d = 0; d < ndim; ++d) {
        g.base += start[d] * strides[d];
        if (shape[d] == 1) continue;
        if (n > 0 && str[n - 1] == shape[d] * strides[d]) {  // axis d spanned: contiguous pair
            ext[n - 1] *= shape[d];
            str[n - 1] = strides[d];
        } else {
            ext[n] = shape[d];
            str[n] = strides[d];
            ++n;
        }
    }
    // the row is the last axis when it has stride 1 (always, unless every extent was 1)
    g.row_len = 1;
    if (n > 0 && str[n - 1] == 1) g.row_len = ext[--n];
    g.rows = 1;
    g.n_outer = n;
    for (int d = 0; d < n; ++d) {
        g.shape[d] = ext[d];
        g.stride[d] = str[d];
        g.rows *= ext[d];
    }
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_pointwise(in, out, g, prog, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "pointwise launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

// ---- two-array arithmetic (an extension; arithmetic.hip) ----------------------------------------

int zt_arithmetic_is_compatible(int op, int dtype_a, int dtype_b, int dtype_out) {
    if (op < ZT_AR_ADD || op > ZT_AR_ABSOLUTE_DIFFERENCE)
        return fail(ZT_ERR_INVALID_PARAMETERS, "unknown arithmetic operator %d", op);
    for (int d : {dtype_a, dtype_b, dtype_out})
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
    return ZT_OK;
}

int zt_arithmetic_memory_per_chunk(int op, int dtype_a, int dtype_b, int dtype_out,
                                   const int64_t* chunk_shape, int ndim, uint64_t* bytes) {
    if (int rc = zt_arithmetic_is_compatible(op, dtype_a, dtype_b, dtype_out)) return rc;
    if (int rc = check_shape(chunk_shape, ndim, "chunk_shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    *bytes = (uint64_t)numel(chunk_shape, ndim) *
             (zt::dtype_size(dtype_a) + zt::dtype_size(dtype_b) + zt::dtype_size(dtype_out));
    return ZT_OK;
}

int zt_arithmetic_apply(zt_ctx* ctx, int op, int dtype_a, const void* a, int dtype_b,
                        const void* b, int64_t n, int dtype_out, void* out) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_arithmetic_is_compatible(op, dtype_a, dtype_b, dtype_out)) return rc;
    if (n < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative element count");
    if (n == 0) return ZT_OK;
    if (!a || !b || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (((uintptr_t)a % zt::dtype_size(dtype_a)) != 0 ||
        ((uintptr_t)b % zt::dtype_size(dtype_b)) != 0 ||
        ((uintptr_t)out % zt::dtype_size(dtype_out)) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_arithmetic(a, dtype_a, b, dtype_b, out, dtype_out, n, op, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "arithmetic launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

// ---- connected-component labelling (an extension; connected.hip) --------------------------------

static_assert(ZT_CC_TILE_Z == zt::kCcTileZ && ZT_CC_TILE_Y == zt::kCcTileY &&
                  ZT_CC_TILE_X == zt::kCcTileX,
              "the public header and the kernels agree on the tile");

namespace {

// the largest label an integer output type holds; 0 for bool and the float types
uint64_t cc_label_max(int dtype) {
    switch (dtype) {
    case ZT_INT8: return 0x7Full;
    case ZT_INT16: return 0x7FFFull;
    case ZT_INT32: return 0x7FFFFFFFull;
    case ZT_INT64: return 0x7FFFFFFFFFFFFFFFull;
    case ZT_UINT8: return 0xFFull;
    case ZT_UINT16: return 0xFFFFull;
    case ZT_UINT32: return 0xFFFFFFFFull;
    case ZT_UINT64: return ~0ull;
    default: return 0;
    }
}

}  // namespace

int zt_connected_components_is_compatible(int dtype_in, int dtype_out) {
    for (int d : {dtype_in, dtype_out})
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
    if (cc_label_max(dtype_out) == 0)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "connected_components: labels need an integer output type, not %s",
                    dtype_name(dtype_out));
    return ZT_OK;
}

int zt_connected_components_memory(int dtype_in, int dtype_out, const int64_t* shape, int ndim,
                                   uint64_t* bytes) {
    if (int rc = zt_connected_components_is_compatible(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    const int64_t n = numel(shape, ndim);
    *bytes = n == 0 ? 0
                    : (uint64_t)n * (zt::dtype_size(dtype_in) + zt::dtype_size(dtype_out)) +
                          zt::cc_scratch_bytes(n, zt::cc_index64(n), ndim);
    return ZT_OK;
}

int zt_connected_components_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                        void* out, const int64_t* shape, int ndim,
                                        int connectivity, uint64_t* count) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_connected_components_is_compatible(dtype_in, dtype_out)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (connectivity < 1 || connectivity > ndim)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "connected_components: connectivity %d not in [1, %d]", connectivity, ndim);
    if (count) *count = 0;
    const int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    if (n > zt::kCcMaxElems)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "connected_components: %lld elements are more than %lld", (long long)n,
                    (long long)zt::kCcMaxElems);
    int64_t tiles = 1;
    for (int d = 0; d < ndim; ++d) {
        const int t = d == ndim - 1 ? ZT_CC_TILE_X : d == ndim - 2 ? ZT_CC_TILE_Y
                      : d == ndim - 3 ? ZT_CC_TILE_Z : 1;
        tiles *= (shape[d] + t - 1) / t;
    }
    if (tiles > 0x7FFFFFFFll)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "connected_components: %lld tiles are more than one launch holds",
                    (long long)tiles);
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (in == out) return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    if (((uintptr_t)in % zt::dtype_size(dtype_in)) != 0 ||
        ((uintptr_t)out % zt::dtype_size(dtype_out)) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    DeviceGuard guard(ctx->device);
    const bool idx64 = zt::cc_index64(n);
    if (int rc = ctx->ensure_scratch((size_t)zt::cc_scratch_bytes(n, idx64, ndim))) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_cc_label(in, dtype_in, shape, ndim, connectivity, idx64,
                                       ctx->scratch, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "connected components launch");
    // K comes back before anything is written: labels never wrap
    uint64_t k = 0;
    ZT_HIP(hipMemcpyAsync(&k, zt::cc_count_ptr(ctx->scratch, n, idx64), sizeof(k),
                          hipMemcpyDeviceToHost, ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    if (k > cc_label_max(dtype_out))
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "connected_components: %llu components do not fit %s", (unsigned long long)k,
                    dtype_name(dtype_out));
    e = zt::launch_cc_write(ctx->scratch, n, idx64, out, dtype_out, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "connected components write launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (count) *count = k;
    return ZT_OK;
}

// ---- exact Euclidean distance transform (an extension; distance.hip) -----------------------------

static_assert(ZT_MAX_DIMS == zt::kEdtMaxDims, "zt_edt_host.hpp and the public header agree");

namespace {

// Shape, spacing and limits of a distance transform -> its plan (zt_edt_host.hpp).
int edt_check(const int64_t* shape, const int64_t* spacing, int ndim, zt::EdtPlan* plan) {
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    switch (zt::edt_plan(shape, spacing, ndim, plan)) {
    case zt::kEdtOk: return ZT_OK;
    case zt::kEdtBadSpacing:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "distance_transform: every spacing must be an integer >= 1");
    case zt::kEdtBoundTooLarge:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "distance_transform: the largest squared distance, the sum of spacing^2 * "
                    "(extent - 1)^2, must be below 2^62");
    case zt::kEdtTooManyElems:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "distance_transform: the array has more than %lld elements",
                    (long long)zt::kEdtMaxElems);
    default:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "distance_transform: every extent must be below 2^31");
    }
}

}  // namespace

int zt_distance_transform_is_compatible(int dtype_in, int dtype_out) {
    for (int d : {dtype_in, dtype_out})
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
    if (dtype_out == ZT_BOOL)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "distance_transform: distances need a numeric output type, not bool");
    return ZT_OK;
}

int zt_distance_transform_memory(int dtype_in, int dtype_out, const int64_t* shape,
                                 const int64_t* spacing, int ndim, uint64_t* bytes) {
    if (int rc = zt_distance_transform_is_compatible(dtype_in, dtype_out)) return rc;
    zt::EdtPlan plan;
    if (int rc = edt_check(shape, spacing, ndim, &plan)) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    *bytes = plan.n == 0
                 ? 0
                 : (uint64_t)plan.n * (zt::dtype_size(dtype_in) + zt::dtype_size(dtype_out)) +
                       zt::edt_scratch_bytes(plan.n, zt::edt_work64(plan.work64));
    return ZT_OK;
}

int zt_distance_transform_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                      void* out, const int64_t* shape, const int64_t* spacing,
                                      int ndim, int squared) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_distance_transform_is_compatible(dtype_in, dtype_out)) return rc;
    zt::EdtPlan plan;
    if (int rc = edt_check(shape, spacing, ndim, &plan)) return rc;
    if (plan.n == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (size_t)plan.n * zt::dtype_size(dtype_in);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)plan.n * zt::dtype_size(dtype_out);
    if (a0 < b1 && b0 < a1)
        return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must not overlap");
    if ((a0 % zt::dtype_size(dtype_in)) != 0 || (b0 % zt::dtype_size(dtype_out)) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    DeviceGuard guard(ctx->device);
    const bool work64 = zt::edt_work64(plan.work64);
    if (int rc = ctx->ensure_scratch((size_t)zt::edt_scratch_bytes(plan.n, work64))) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_edt(in, dtype_in, shape, ndim, plan.weight, work64, ctx->scratch, out,
                                  dtype_out, squared != 0, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "distance transform launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

// ---- per-label statistics and the label size filter (extensions; labels.hip) ---------------------

static_assert(ZT_MAX_DIMS == zt::kLblMaxDims, "zt_labels_host.hpp and the public header agree");
static_assert(ZT_LABELS_TILE_ROWS == zt::kLblTileRows, "the public header names the tile");

namespace {

int lbl_fail(int status, int64_t n_labels) {
    switch (status) {
    case zt::kLblOk: return ZT_OK;
    case zt::kLblBadLabels:
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_statistics: n_labels %lld not in [0, %lld]",
                    (long long)n_labels, (long long)zt::kLblMaxLabels);
    case zt::kLblBadOrigin:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_statistics: every origin must be >= 0 and origin + extent an int64");
    case zt::kLblTooManyElems:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_statistics: the box has more than %lld elements",
                    (long long)zt::kLblMaxElems);
    case zt::kLblSumWraps:
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_statistics: elements * (origin + extent) must be below 2^64, so that "
                    "no coordinate sum wraps");
    default:
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_statistics: the state is too large");
    }
}

int lbl_state_ok(const void* state) {
    if (!state || ((uintptr_t)state % 8) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "the label statistics state is device memory, 8-byte aligned");
    return ZT_OK;
}

int lbl_ndim_ok(int ndim) {
    if (ndim < 1 || ndim > ZT_MAX_DIMS)
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_statistics: ndim %d not in [1, %d]", ndim,
                    ZT_MAX_DIMS);
    return ZT_OK;
}

}  // namespace

int zt_label_statistics_is_compatible(int dtype_labels, int dtype_intensity) {
    if (!valid_dtype(dtype_labels))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype_labels);
    if (cc_label_max(dtype_labels) == 0)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "label_statistics: labels need an integer type, not %s",
                    dtype_name(dtype_labels));
    if (dtype_intensity == ZT_NO_DTYPE) return ZT_OK;
    if (!valid_dtype(dtype_intensity))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d",
                    dtype_intensity);
    if (dtype_intensity == ZT_BOOL)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "label_statistics: intensities need a numeric type, not bool");
    return ZT_OK;
}

int zt_label_statistics_state_bytes(int ndim, int64_t n_labels, int with_intensity,
                                    uint64_t* bytes) {
    if (int rc = lbl_ndim_ok(ndim)) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    zt::LblPlan plan;
    if (int rc = lbl_fail(zt::lbl_state(ndim, n_labels, with_intensity != 0, false, &plan),
                          n_labels))
        return rc;
    *bytes = plan.state_bytes;
    return ZT_OK;
}

int zt_label_statistics_init(zt_ctx* ctx, int ndim, int64_t n_labels, int with_intensity,
                             void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = lbl_ndim_ok(ndim)) return rc;
    zt::LblPlan plan;
    if (int rc = lbl_fail(zt::lbl_state(ndim, n_labels, with_intensity != 0, false, &plan),
                          n_labels))
        return rc;
    if (int rc = lbl_state_ok(state)) return rc;
    DeviceGuard guard(ctx->device);
    hipError_t e = zt::launch_lbl_init(state, ndim, n_labels, with_intensity != 0, false, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "label statistics init launch");
    return ZT_OK;
}

int zt_label_statistics_accumulate(zt_ctx* ctx, int dtype_labels, const void* labels,
                                   int dtype_intensity, const void* intensity,
                                   const int64_t* box_shape, const int64_t* origin, int ndim,
                                   int64_t n_labels, void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_label_statistics_is_compatible(dtype_labels, dtype_intensity)) return rc;
    if (int rc = check_shape(box_shape, ndim, "box_shape")) return rc;
    if ((dtype_intensity == ZT_NO_DTYPE) != (intensity == nullptr))
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_statistics: an intensity array and its data type go together");
    zt::LblPlan plan;
    if (int rc = lbl_fail(zt::lbl_plan(box_shape, origin, ndim, n_labels, intensity != nullptr,
                                       false, &plan),
                          n_labels))
        return rc;
    if (int rc = lbl_state_ok(state)) return rc;
    if (plan.n == 0) return ZT_OK;
    if (!labels) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (((uintptr_t)labels % zt::dtype_size(dtype_labels)) != 0 ||
        (intensity && ((uintptr_t)intensity % zt::dtype_size(dtype_intensity)) != 0))
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_lbl_accumulate(labels, dtype_labels, intensity, dtype_intensity,
                                             box_shape, origin, ndim, n_labels, false, state,
                                             ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "label statistics launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int zt_label_statistics_finish(zt_ctx* ctx, const void* state, int ndim, int64_t n_labels,
                               int with_intensity, uint64_t* host_state, uint64_t* invalid) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = lbl_ndim_ok(ndim)) return rc;
    zt::LblPlan plan;
    if (int rc = lbl_fail(zt::lbl_state(ndim, n_labels, with_intensity != 0, false, &plan),
                          n_labels))
        return rc;
    if (int rc = lbl_state_ok(state)) return rc;
    DeviceGuard guard(ctx->device);
    uint64_t bad = 0;
    const uint64_t* words = static_cast<const uint64_t*>(state);
    if (host_state)
        ZT_HIP(hipMemcpyAsync(host_state, state, (size_t)plan.state_bytes, hipMemcpyDeviceToHost,
                              ctx->cur));
    ZT_HIP(hipMemcpyAsync(&bad, words + plan.state_words - 1, sizeof bad, hipMemcpyDeviceToHost,
                          ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    if (invalid) *invalid = bad;
    if (bad)
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_statistics: %llu elements outside [0, %lld]",
                    (unsigned long long)bad, (long long)n_labels);
    return ZT_OK;
}

int zt_label_size_filter_is_compatible(int dtype_in, int dtype_out) {
    for (int d : {dtype_in, dtype_out}) {
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
        if (cc_label_max(d) == 0)
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                        "label_size_filter: labels need an integer type, not %s", dtype_name(d));
    }
    return ZT_OK;
}

namespace {

int lsf_sizes_ok(int64_t min_size, int64_t max_size) {
    if (min_size < 1)
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_size_filter: min_size %lld is below 1",
                    (long long)min_size);
    if (max_size >= 0 && max_size < min_size)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_size_filter: max_size %lld is below min_size %lld", (long long)max_size,
                    (long long)min_size);
    return ZT_OK;
}

int lsf_elems(const int64_t* shape, int ndim, int64_t* n) {
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    zt::LblPlan plan;
    if (int rc = lbl_fail(zt::lbl_plan(shape, nullptr, ndim, 0, false, true, &plan), 0)) return rc;
    *n = plan.n;
    return ZT_OK;
}

}  // namespace

int zt_label_size_filter_memory(int dtype_in, int dtype_out, const int64_t* shape, int ndim,
                                int64_t n_labels, uint64_t* bytes) {
    if (int rc = zt_label_size_filter_is_compatible(dtype_in, dtype_out)) return rc;
    int64_t n = 0;
    if (int rc = lsf_elems(shape, ndim, &n)) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    uint64_t scratch = 0;
    if (int rc = lbl_fail(zt::lbl_filter_scratch(n_labels, &scratch), n_labels)) return rc;
    *bytes = n == 0 ? 0
                    : (uint64_t)n * (zt::dtype_size(dtype_in) + zt::dtype_size(dtype_out)) + scratch;
    return ZT_OK;
}

int zt_label_size_filter_apply_array(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out,
                                     void* out, const int64_t* shape, int ndim, int64_t min_size,
                                     int64_t max_size, int relabel, uint64_t* kept) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_label_size_filter_is_compatible(dtype_in, dtype_out)) return rc;
    if (int rc = lsf_sizes_ok(min_size, max_size)) return rc;
    int64_t n = 0;
    if (int rc = lsf_elems(shape, ndim, &n)) return rc;
    if (kept) *kept = 0;
    if (n == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (size_t)n * zt::dtype_size(dtype_in);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)n * zt::dtype_size(dtype_out);
    if (a0 < b1 && b0 < a1)
        return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must not overlap");
    if ((a0 % zt::dtype_size(dtype_in)) != 0 || (b0 % zt::dtype_size(dtype_out)) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    DeviceGuard guard(ctx->device);
    // 1. the largest label (and the smallest: a negative element is refused here)
    if (int rc = ctx->ensure_scratch(16)) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_range_init(ctx->scratch, ctx->cur);
    if (e == hipSuccess) e = zt::launch_range_accumulate(in, dtype_in, n, ctx->scratch, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "label size filter range launch");
    uint64_t keys[2] = {0, 0}, lo = 0, hi = 0;
    ZT_HIP(hipMemcpyAsync(keys, ctx->scratch, sizeof keys, hipMemcpyDeviceToHost, ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    zt::range_decode(dtype_in, keys[0], &lo);
    zt::range_decode(dtype_in, keys[1], &hi);
    const int bits = 8 * (int)zt::dtype_size(dtype_in);
    if (dtype_in <= ZT_INT64 && ((lo >> (bits - 1)) & 1))
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_size_filter: the labels have a negative element");
    if (hi > (uint64_t)zt::kLblMaxLabels)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "label_size_filter: the largest label %llu is above %lld",
                    (unsigned long long)hi, (long long)zt::kLblMaxLabels);
    const int64_t K = (int64_t)hi;
    // 2. counts, 3. keep and scan
    uint64_t scratch_bytes = 0;
    if (int rc = lbl_fail(zt::lbl_filter_scratch(K, &scratch_bytes), K)) return rc;
    if (int rc = ctx->ensure_scratch((size_t)scratch_bytes)) return rc;
    uint8_t* base = static_cast<uint8_t*>(ctx->scratch);
    void* counts = base;
    void* remap = base + 8 * ((size_t)K + 2);
    void* tail = base + scratch_bytes - 16;
    e = zt::launch_lbl_init(counts, 1, K, false, true, ctx->cur);
    if (e == hipSuccess)
        e = zt::launch_lbl_accumulate(in, dtype_in, nullptr, ZT_NO_DTYPE, shape, nullptr, ndim, K,
                                      true, counts, ctx->cur);
    if (e == hipSuccess)
        e = zt::launch_lbl_keep_scan(counts, K, (uint64_t)min_size,
                                     max_size < 0 ? ~0ull : (uint64_t)max_size, relabel != 0, remap,
                                     tail, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "label size filter launch");
    // K' and the largest label kept come back before anything is written: labels never wrap
    uint64_t res[2] = {0, 0};
    ZT_HIP(hipMemcpyAsync(res, tail, sizeof res, hipMemcpyDeviceToHost, ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    const uint64_t largest = relabel ? res[0] : res[1];
    if (largest > cc_label_max(dtype_out))
        return fail(ZT_ERR_INVALID_PARAMETERS, "label_size_filter: the largest label %llu does not fit %s",
                    (unsigned long long)largest, dtype_name(dtype_out));
    // 4. out[i] = remap[in[i]]
    e = zt::launch_lbl_gather(in, dtype_in, remap, out, dtype_out, n, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "label size filter write launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (kept) *kept = res[0];
    return ZT_OK;
}

// ---- morphological reconstruction (an extension; reconstruct.hip) --------------------------------

static_assert(ZT_REC_TILE_Z == zt::kRecTileZ && ZT_REC_TILE_Y == zt::kRecTileY &&
                  ZT_REC_TILE_X == zt::kRecTileX && ZT_REC_BATCH == zt::kRecBatch,
              "the public header and the kernels agree on the tile and the batch");
static_assert(ZT_REC_MARKER == zt::kRecMarker && ZT_REC_FILL_HOLES == zt::kRecFillHoles &&
                  ZT_REC_H_MAXIMA == zt::kRecHMaxima && ZT_REC_H_MINIMA == zt::kRecHMinima,
              "marker modes");
static_assert(zt::kRecBatch * sizeof(uint32_t) <= zt::kRecTail, "the flag words fit the tail");

int zt_reconstruction_is_compatible(int dtype_mask, int dtype_marker, int marker_mode) {
    for (int d : {dtype_mask, dtype_marker})
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
    if (marker_mode < ZT_REC_MARKER || marker_mode > ZT_REC_H_MINIMA)
        return fail(ZT_ERR_INVALID_PARAMETERS, "reconstruction: unknown marker mode %d",
                    marker_mode);
    if (marker_mode == ZT_REC_MARKER && dtype_marker != dtype_mask)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "reconstruction: the marker is %s and the mask %s; they need one data type",
                    dtype_name(dtype_marker), dtype_name(dtype_mask));
    if ((marker_mode == ZT_REC_H_MAXIMA || marker_mode == ZT_REC_H_MINIMA) &&
        dtype_mask == ZT_BOOL)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "reconstruction: h_maxima and h_minima need a numeric type, not bool");
    return ZT_OK;
}

int zt_reconstruction_memory(int dtype, int marker_mode, const int64_t* shape, int ndim,
                             uint64_t* bytes) {
    if (int rc = zt_reconstruction_is_compatible(dtype, dtype, marker_mode)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    const int64_t n = numel(shape, ndim);
    zt::RecGeom geom;
    if (n != 0 && !zt::rec_geom(shape, ndim, &geom))
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "reconstruction: rank %d is supported only when every axis in front of the "
                    "innermost three has extent 1", ndim);
    const int esz = (int)zt::dtype_size(dtype);
    const uint64_t arrays = marker_mode == ZT_REC_MARKER ? 3 : 2;  // mask, (marker,) output
    *bytes = n == 0 ? 0 : arrays * (uint64_t)n * esz + zt::rec_scratch_bytes(n, esz);
    return ZT_OK;
}

int zt_reconstruction_apply_array(zt_ctx* ctx, int dtype, const void* mask, const void* marker,
                                  int marker_mode, double h, void* out, const int64_t* shape,
                                  int ndim, int connectivity, int method, uint64_t* rounds) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_reconstruction_is_compatible(dtype, dtype, marker_mode)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (connectivity < 1 || connectivity > ndim)
        return fail(ZT_ERR_INVALID_PARAMETERS, "reconstruction: connectivity %d not in [1, %d]",
                    connectivity, ndim);
    if (marker_mode == ZT_REC_MARKER && method != ZT_REC_DILATION && method != ZT_REC_EROSION)
        return fail(ZT_ERR_INVALID_PARAMETERS, "reconstruction: unknown method %d", method);
    const bool h_mode = marker_mode == ZT_REC_H_MAXIMA || marker_mode == ZT_REC_H_MINIMA;
    if (h_mode && !(std::isfinite(h) && h > 0))
        return fail(ZT_ERR_INVALID_PARAMETERS, "reconstruction: h must be finite and > 0");
    if (rounds) *rounds = 0;
    const int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    zt::RecGeom geom;
    if (!zt::rec_geom(shape, ndim, &geom))
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "reconstruction: rank %d is supported only when every axis in front of the "
                    "innermost three has extent 1", ndim);
    if (n > zt::kRecMaxElems)
        return fail(ZT_ERR_INVALID_PARAMETERS, "reconstruction: %lld elements are more than %lld",
                    (long long)n, (long long)zt::kRecMaxElems);
    if (zt::rec_tiles(geom) > 0x7FFFFFFFll)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "reconstruction: %lld tiles are more than one launch holds",
                    (long long)zt::rec_tiles(geom));
    const bool two = marker_mode == ZT_REC_MARKER;
    if (!mask || !out || (two && !marker))
        return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (mask == out || (two && marker == out))
        return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    const int esz = (int)zt::dtype_size(dtype);
    if (((uintptr_t)mask % esz) != 0 || ((uintptr_t)out % esz) != 0 ||
        (two && ((uintptr_t)marker % esz) != 0))
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    const bool erosion = two ? method == ZT_REC_EROSION : marker_mode != ZT_REC_H_MAXIMA;
    const int sweeps = zt::rec_tile_sweeps();
    DeviceGuard guard(ctx->device);
    if (int rc = ctx->ensure_scratch((size_t)zt::rec_scratch_bytes(n, esz))) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    // buf[0] is the scratch array, buf[1] is `out`: round r reads buf[r % 2] and writes the other
    void* buf[2] = {ctx->scratch, out};
    uint32_t* flags = zt::rec_flags_ptr(ctx->scratch, n, esz);
    hipError_t e = zt::launch_rec_init(mask, marker, buf[0], dtype, geom, marker_mode, h, erosion,
                                       ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "reconstruction init launch");
    // Every round but the last raises at least one element, so n + 1 rounds are a bound. Once a
    // round has changed nothing the two buffers are equal; the rest of its batch does nothing.
    uint64_t done = 0;
    for (;;) {
        ZT_HIP(hipMemsetAsync(flags, 0, zt::kRecBatch * sizeof(uint32_t), ctx->cur));
        for (int k = 0; k < zt::kRecBatch; ++k) {
            const uint64_t r = done + k;
            e = zt::launch_rec_round(buf[r % 2], mask, buf[(r + 1) % 2], dtype, geom,
                                     connectivity, erosion, sweeps, flags + k,
                                     k ? flags + k - 1 : nullptr, ctx->cur);
            if (e != hipSuccess) return hip_fail(e, "reconstruction round launch");
        }
        uint32_t host[zt::kRecBatch];
        ZT_HIP(hipMemcpyAsync(host, flags, sizeof host, hipMemcpyDeviceToHost, ctx->cur));
        ZT_HIP(hipStreamSynchronize(ctx->cur));
        int quiet = -1;
        for (int k = 0; k < zt::kRecBatch && quiet < 0; ++k)
            if (host[k] == 0) quiet = k;
        if (quiet >= 0) {
            done += (uint64_t)quiet + 1;
            break;
        }
        done += zt::kRecBatch;
        if (done > (uint64_t)n)
            return fail(ZT_ERR_OTHER, "reconstruction: no fixed point after %llu rounds of %lld "
                        "elements", (unsigned long long)done, (long long)n);
    }
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (rounds) *rounds = done;
    return ZT_OK;
}

// ---- seeded watershed (an extension; watershed.hip) ---------------------------------------------

namespace {

// what zt_watershed_memory and zt_watershed_apply_array refuse alike; n = 0 passes
int ws_check(const int64_t* shape, int ndim, int connectivity, zt::RecGeom* geom) {
    if (connectivity < 1 || connectivity > ndim)
        return fail(ZT_ERR_INVALID_PARAMETERS, "watershed: connectivity %d not in [1, %d]",
                    connectivity, ndim);
    const int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    if (!zt::rec_geom(shape, ndim, geom))
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "watershed: rank %d is supported only when every axis in front of the "
                    "innermost three has extent 1", ndim);
    if (n > zt::kWsMaxElems)
        return fail(ZT_ERR_INVALID_PARAMETERS, "watershed: %lld elements are more than %lld",
                    (long long)n, (long long)zt::kWsMaxElems);
    if (zt::rec_tiles(*geom) > 0x7FFFFFFFll)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "watershed: %lld tiles are more than one launch holds",
                    (long long)zt::rec_tiles(*geom));
    return ZT_OK;
}

// Rounds in batches of kRecBatch, each with its own flag word, until the first that raised none:
// `launch(r, flag, prev)` enqueues round r. *count = the rounds up to and including that one;
// more than `cap` of them is ZT_ERR_OTHER.
extern "C++" {
template <typename Launch>
int ws_rounds(zt_ctx* ctx, uint32_t* flags, uint64_t cap, const char* what, int64_t* count,
              Launch launch) {
    uint64_t done = 0;
    for (;;) {
        ZT_HIP(hipMemsetAsync(flags, 0, zt::kRecBatch * sizeof(uint32_t), ctx->cur));
        for (int k = 0; k < zt::kRecBatch; ++k) {
            const hipError_t e = launch(done + k, flags + k, k ? flags + k - 1 : nullptr);
            if (e != hipSuccess) return hip_fail(e, what);
        }
        uint32_t host[zt::kRecBatch];
        ZT_HIP(hipMemcpyAsync(host, flags, sizeof host, hipMemcpyDeviceToHost, ctx->cur));
        ZT_HIP(hipStreamSynchronize(ctx->cur));
        for (int k = 0; k < zt::kRecBatch; ++k)
            if (host[k] == 0) {
                *count = (int64_t)(done + k + 1);
                return ZT_OK;
            }
        done += zt::kRecBatch;
        if (done > cap)
            return fail(ZT_ERR_OTHER, "watershed: %s: no fixed point after %llu rounds (cap %llu)",
                        what, (unsigned long long)done, (unsigned long long)cap);
    }
}
}  // extern "C++"

}  // namespace

int zt_watershed_is_compatible(int dtype_relief, int dtype_seeds) {
    for (int d : {dtype_relief, dtype_seeds})
        if (!valid_dtype(d))
            return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", d);
    if (cc_label_max(dtype_seeds) == 0)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "watershed: seeds and labels need an integer type, not %s",
                    dtype_name(dtype_seeds));
    return ZT_OK;
}

int zt_watershed_memory(int dtype_relief, int dtype_seeds, const int64_t* shape, int ndim,
                        int connectivity, int foreground_only, uint64_t* bytes) {
    if (int rc = zt_watershed_is_compatible(dtype_relief, dtype_seeds)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!bytes) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    zt::RecGeom geom;
    if (int rc = ws_check(shape, ndim, connectivity, &geom)) return rc;
    const int64_t n = numel(shape, ndim);
    const int esz = (int)zt::dtype_size(dtype_relief), ssz = (int)zt::dtype_size(dtype_seeds);
    // relief, seeds, output, scratch
    *bytes = n == 0 ? 0
                    : (uint64_t)n * esz + 2 * (uint64_t)n * ssz +
                          zt::ws_scratch_bytes(n, esz, foreground_only != 0);
    return ZT_OK;
}

int zt_watershed_apply_array(zt_ctx* ctx, int dtype_relief, const void* relief, int dtype_seeds,
                             const void* seeds, void* out, const int64_t* shape, int ndim,
                             int connectivity, int descending, int foreground_only,
                             int64_t rounds[3]) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_watershed_is_compatible(dtype_relief, dtype_seeds)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    zt::RecGeom geom;
    if (int rc = ws_check(shape, ndim, connectivity, &geom)) return rc;
    int64_t counts[3] = {0, 0, 0};
    if (rounds) rounds[0] = rounds[1] = rounds[2] = 0;
    const int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    if (!relief || !seeds || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (relief == out || seeds == out)
        return fail(ZT_ERR_INVALID_PARAMETERS, "input and output must differ");
    const int esz = (int)zt::dtype_size(dtype_relief), ssz = (int)zt::dtype_size(dtype_seeds);
    if (((uintptr_t)relief % esz) != 0 || ((uintptr_t)seeds % ssz) != 0 ||
        ((uintptr_t)out % ssz) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    const bool desc = descending != 0, fg = foreground_only != 0;
    const int sweeps = zt::rec_tile_sweeps();
    DeviceGuard guard(ctx->device);
    const uint64_t scratch_bytes = zt::ws_scratch_bytes(n, esz, fg);
    if (int rc = ctx->ensure_scratch((size_t)scratch_bytes)) return rc;
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    // the scratch: c[0], c[1], (the relief copy,) d[0], d[1], the flag words
    uint8_t* at = static_cast<uint8_t*>(ctx->scratch);
    const uint64_t cbytes = zt::ws_pad16((uint64_t)n * esz), dbytes = zt::ws_pad16((uint64_t)n * 4);
    void* c[2] = {at, at + cbytes};
    at += 2 * cbytes;
    void* domain = fg ? at : nullptr;
    if (fg) at += cbytes;
    uint32_t* d[2] = {reinterpret_cast<uint32_t*>(at), reinterpret_cast<uint32_t*>(at + dbytes)};
    uint32_t* flags = reinterpret_cast<uint32_t*>(at + 2 * dbytes);
    hipStream_t s = ctx->cur;
    hipError_t e = zt::launch_ws_init(relief, dtype_relief, seeds, dtype_seeds, c[0], domain, d[0],
                                      n, desc, s);
    if (e != hipSuccess) return hip_fail(e, "watershed init launch");
    // 1. pass values: the reconstruction of J0 under the relief (by erosion; flooding from the
    // maxima is the erosion on complemented keys, which is the dilation). At most n + 1 rounds
    // (DESIGN.md §3.16); once a round has changed nothing c[0] and c[1] are equal.
    const void* under = fg ? domain : relief;
    if (int rc = ws_rounds(ctx, flags, (uint64_t)n, "pass value rounds", &counts[0],
                           [&](uint64_t r, uint32_t* flag, const uint32_t* prev) {
                               return zt::launch_rec_round(c[r % 2], under, c[(r + 1) % 2],
                                                           dtype_relief, geom, connectivity, !desc,
                                                           sweeps, flag, prev, s);
                           }))
        return rc;
    // 2. plateau distances, at most n + 1 rounds; afterwards d[0] and d[1] are equal
    if (int rc = ws_rounds(ctx, flags, (uint64_t)n, "distance rounds", &counts[1],
                           [&](uint64_t r, uint32_t* flag, const uint32_t* prev) {
                               return zt::launch_ws_dist_round(c[0], dtype_relief, d[r % 2],
                                                               d[(r + 1) % 2], geom, connectivity,
                                                               desc, sweeps, flag, prev, s);
                           }))
        return rc;
    // 3. parents, from d[0] into d[1]; then the jumps alternate between the two d arrays, the
    // distances being done with
    e = zt::launch_ws_parent(c[0], dtype_relief, d[0], seeds, dtype_seeds, d[1], geom,
                             connectivity, desc, s);
    if (e != hipSuccess) return hip_fail(e, "watershed parent launch");
    uint32_t* p[2] = {d[1], d[0]};
    if (int rc = ws_rounds(ctx, flags, (uint64_t)zt::ws_jump_cap(n), "jumps", &counts[2],
                           [&](uint64_t r, uint32_t* flag, const uint32_t* prev) {
                               return zt::launch_ws_jump(p[r % 2], p[(r + 1) % 2], n, flag, prev,
                                                         s);
                           }))
        return rc;
    // 4. the round that changed nothing copied its input: both arrays hold the roots
    e = zt::launch_ws_gather(p[0], seeds, dtype_seeds, out, n, s);
    if (e != hipSuccess) return hip_fail(e, "watershed gather launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    if (rounds)
        for (int k = 0; k < 3; ++k) rounds[k] = counts[k];
    return ZT_OK;
}

// ---- zarrs_info reductions (range.rs, histogram.rs) --------------------------------------------

namespace {

// the 12 numeric types; bool is `unimplemented!` in the reference (range.rs:92-95,
// histogram.rs:32-35)
int info_dtype_ok(int dtype) {
    if (!valid_dtype(dtype))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype);
    if (dtype == ZT_BOOL) return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type bool");
    return ZT_OK;
}

int info_run_ok(int dtype, const void* in, int64_t n) {
    if (n < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative element count");
    if (n > 0 && !in) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    if (((uintptr_t)in % zt::dtype_size(dtype)) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "data pointers must be element aligned");
    return ZT_OK;
}

int histogram_args_ok(int64_t n_bins, double mn, double mx) {
    if (n_bins < 1 || n_bins > zt::kInfoMaxBins)
        return fail(ZT_ERR_INVALID_PARAMETERS, "n_bins %lld not in [1, %lld]", (long long)n_bins,
                    (long long)zt::kInfoMaxBins);
    if (!std::isfinite(mn) || !std::isfinite(mx))
        return fail(ZT_ERR_INVALID_PARAMETERS, "histogram min and max must be finite");
    return ZT_OK;
}

}  // namespace

int zt_range_is_compatible(int dtype) { return info_dtype_ok(dtype); }
int zt_histogram_is_compatible(int dtype) { return info_dtype_ok(dtype); }

int zt_range_init(zt_ctx* ctx, void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (!state || ((uintptr_t)state % 8) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "the range state is 16 device bytes, 8-byte aligned");
    DeviceGuard guard(ctx->device);
    hipError_t e = zt::launch_range_init(state, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "range init launch");
    return ZT_OK;
}

int zt_range_accumulate(zt_ctx* ctx, int dtype, const void* in, int64_t n, void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = info_dtype_ok(dtype)) return rc;
    if (int rc = info_run_ok(dtype, in, n)) return rc;
    if (!state || ((uintptr_t)state % 8) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "the range state is 16 device bytes, 8-byte aligned");
    if (n == 0) return ZT_OK;
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_range_accumulate(in, dtype, n, state, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "range launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int zt_range_finish(zt_ctx* ctx, int dtype, const void* state, uint64_t* min_bits,
                    uint64_t* max_bits, int* none) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = info_dtype_ok(dtype)) return rc;
    if (!state || !min_bits || !max_bits || !none)
        return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    DeviceGuard guard(ctx->device);
    uint64_t keys[2] = {0, 0};
    ZT_HIP(hipMemcpyAsync(keys, state, sizeof keys, hipMemcpyDeviceToHost, ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    *none = keys[0] > keys[1] ? 1 : 0;
    *min_bits = *max_bits = 0;
    if (!*none) {
        zt::range_decode(dtype, keys[0], min_bits);
        zt::range_decode(dtype, keys[1], max_bits);
    }
    return ZT_OK;
}

int zt_histogram_accumulate(zt_ctx* ctx, int dtype, const void* in, int64_t n, int64_t n_bins,
                            double min, double max, uint64_t* hist) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = info_dtype_ok(dtype)) return rc;
    if (int rc = histogram_args_ok(n_bins, min, max)) return rc;
    if (int rc = info_run_ok(dtype, in, n)) return rc;
    if (!hist || ((uintptr_t)hist % 8) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "hist is n_bins device uint64, 8-byte aligned");
    if (n == 0) return ZT_OK;
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_histogram_accumulate(in, dtype, n, n_bins, min, max, hist, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "histogram launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int zt_histogram_bin_edges(int64_t n_bins, double min, double max, double* edges) {
    if (int rc = histogram_args_ok(n_bins, min, max)) return rc;
    if (!edges) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    const double range = max - min, nb = (double)n_bins;  // histogram.rs:62-68
    for (int64_t i = 0; i <= n_bins; ++i) edges[i] = ((double)i / nb) * range + min;
    return ZT_OK;
}

// ---- zarrs_validate comparison (zarrs_validate.rs:145-147) --------------------------------------

namespace {

int compare_state_ok(const void* state) {
    if (!state || ((uintptr_t)state % 8) != 0)
        return fail(ZT_ERR_INVALID_PARAMETERS,
                    "the compare state is 16 device bytes, 8-byte aligned");
    return ZT_OK;
}

}  // namespace

int zt_compare_init(zt_ctx* ctx, void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = compare_state_ok(state)) return rc;
    DeviceGuard guard(ctx->device);
    hipError_t e = zt::launch_compare_init(state, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "compare init launch");
    return ZT_OK;
}

int zt_compare_accumulate(zt_ctx* ctx, int dtype, const void* a, const void* b, int64_t n,
                          int64_t base, void* state) {
    if (int rc = begin_call(ctx)) return rc;
    if (!valid_dtype(dtype))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype);
    if (int rc = info_run_ok(dtype, a, n)) return rc;
    if (int rc = info_run_ok(dtype, b, n)) return rc;
    if (base < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative base index");
    if (int rc = compare_state_ok(state)) return rc;
    if (n == 0) return ZT_OK;
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_compare_accumulate(a, b, (int)zt::dtype_size(dtype), n, base, state,
                                                 ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "compare launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int zt_compare_finish(zt_ctx* ctx, const void* state, uint64_t* n_diff, int64_t* first) {
    if (int rc = begin_call(ctx)) return rc;
    if (!state || !n_diff || !first) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    DeviceGuard guard(ctx->device);
    uint64_t words[2] = {0, 0};
    ZT_HIP(hipMemcpyAsync(words, state, sizeof words, hipMemcpyDeviceToHost, ctx->cur));
    ZT_HIP(hipStreamSynchronize(ctx->cur));
    *n_diff = words[0];
    *first = words[1] == ~(uint64_t)0 ? -1 : (int64_t)words[1];
    return ZT_OK;
}

// ---- chunk occupancy (zarrs store_empty_chunks = false) -----------------------------------------

int zt_chunk_occupancy_is_compatible(int dtype) {
    if (!valid_dtype(dtype))
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "Unsupported data type code %d", dtype);
    return ZT_OK;
}

int zt_chunk_occupancy(zt_ctx* ctx, int dtype, const void* data, const int64_t* shape, int ndim,
                       const int64_t* cell_shape, uint64_t fill_bits, uint8_t* occupied) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_chunk_occupancy_is_compatible(dtype)) return rc;
    if (!shape || !cell_shape || ndim < 1 || ndim > ZT_MAX_DIMS)
        return fail(ZT_ERR_INVALID_PARAMETERS, "shape / cell_shape of 1 to %d axes", ZT_MAX_DIMS);
    int64_t n = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative extent");
        if (cell_shape[d] < 1) return fail(ZT_ERR_INVALID_PARAMETERS, "cell extents must be >= 1");
        if (shape[d] > 0 && n > INT64_MAX / 16 / shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "the box is too large");
        n *= shape[d];
    }
    if (n == 0) return ZT_OK;
    if (int rc = info_run_ok(dtype, data, n)) return rc;
    if (!occupied) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer");
    DeviceGuard guard(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_chunk_occupancy(data, (int)zt::dtype_size(dtype), shape, ndim,
                                              cell_shape, fill_bits, occupied, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "chunk occupancy launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

// ---- downsample ------------------------------------------------------------------------------

int zt_downsample_is_compatible(int dtype_in, int dtype_out, int discrete) {
    if (int rc = dtypes_ok(dtype_in, dtype_out)) return rc;
    if (discrete && dtype_in >= ZT_BFLOAT16)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE,
                    "Unsupported data type %s for discrete (mode) downsampling",
                    dtype_name(dtype_in));
    return ZT_OK;
}

int zt_downsample_output_shape(const int64_t* in_shape, int ndim, const int64_t* stride,
                               int64_t* out_shape) {
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (!stride || !out_shape) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer argument");
    for (int d = 0; d < ndim; ++d) {
        if (stride[d] <= 0) return fail(ZT_ERR_INVALID_PARAMETERS, "stride must be positive");
        out_shape[d] = std::max<int64_t>(in_shape[d] / stride[d], 1);  // downsample.rs:162-168
    }
    return ZT_OK;
}

int zt_downsample_input_subset(const int64_t* in_shape, int ndim, const int64_t* stride,
                               const int64_t* out_start, const int64_t* out_shape,
                               int64_t* in_start, int64_t* in_subset_shape) {
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (!stride || !out_start || !out_shape || !in_start || !in_subset_shape)
        return fail(ZT_ERR_INVALID_PARAMETERS, "null pointer argument");
    for (int d = 0; d < ndim; ++d) {
        if (stride[d] <= 0) return fail(ZT_ERR_INVALID_PARAMETERS, "stride must be positive");
        // downsample.rs:65-69
        int64_t s = out_start[d] * stride[d];
        int64_t e = std::min((out_start[d] + out_shape[d]) * stride[d], in_shape[d]);
        in_start[d] = s;
        in_subset_shape[d] = std::max<int64_t>(e - s, 0);
    }
    return ZT_OK;
}

int zt_downsample_apply_ndarray(zt_ctx* ctx, int dtype_in, const void* in,
                                const int64_t* in_shape, int ndim, const int64_t* stride,
                                int discrete, int dtype_out, void* out) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = zt_downsample_is_compatible(dtype_in, dtype_out, discrete)) return rc;
    if (int rc = check_shape(in_shape, ndim, "in_shape")) return rc;
    if (!stride) return fail(ZT_ERR_INVALID_PARAMETERS, "null stride");
    zt::DSParams p{};
    p.ndim = ndim;
    p.out_numel = 1;
    p.win_numel = 1;
    for (int d = 0; d < ndim; ++d) {
        if (stride[d] <= 0) return fail(ZT_ERR_INVALID_PARAMETERS, "stride must be positive");
        p.in_shape[d] = in_shape[d];
        p.win[d] = std::min(stride[d], in_shape[d]);       // downsample.rs:83-85
        p.out_shape[d] = p.win[d] > 0 ? in_shape[d] / p.win[d] : 0;  // exact_chunks
        p.out_numel *= p.out_shape[d];
        p.win_numel *= p.win[d];
    }
    if (p.out_numel == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
    hipError_t e = zt::launch_downsample(in, dtype_in, out, dtype_out, p, discrete != 0, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "downsample launch");
    if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
    return ZT_OK;
}

int zt_pyramid_level_shapes(const int64_t* shape, int ndim, const int64_t* factor, int max_levels,
                            int64_t* level_shapes, int* n_levels) {
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (!factor || !level_shapes || !n_levels || max_levels < 0)
        return fail(ZT_ERR_INVALID_PARAMETERS, "bad pyramid arguments");
    int64_t cur[ZT_MAX_DIMS];
    std::copy(shape, shape + ndim, cur);
    int n = 0;
    for (int i = 1; i <= max_levels; ++i) {  // zarrs_ome.rs:515
        int64_t nxt[ZT_MAX_DIMS];
        if (int rc = zt_downsample_output_shape(cur, ndim, factor, nxt)) return rc;
        std::copy(nxt, nxt + ndim, level_shapes + (size_t)n * ndim);
        ++n;
        std::copy(nxt, nxt + ndim, cur);
        bool stop = true;  // zarrs_ome.rs:731-737
        for (int d = 0; d < ndim; ++d)
            if (!(factor[d] == 1 || nxt[d] == 1)) stop = false;
        if (stop) break;
    }
    *n_levels = n;
    return ZT_OK;
}

int zt_pyramid_downsample(zt_ctx* ctx, int dtype, const void* level0, const int64_t* shape,
                          int ndim, const int64_t* factor, int max_levels, int discrete,
                          void* const* level_ptrs, int* levels_written) {
    if (int rc = begin_call(ctx)) return rc;
    if (!level_ptrs || !levels_written) return fail(ZT_ERR_INVALID_PARAMETERS, "null pointers");
    std::vector<int64_t> shapes((size_t)std::max(max_levels, 1) * ZT_MAX_DIMS);
    int n = 0;
    if (int rc = zt_pyramid_level_shapes(shape, ndim, factor, max_levels, shapes.data(), &n))
        return rc;
    const void* src = level0;
    int64_t cur[ZT_MAX_DIMS];
    std::copy(shape, shape + ndim, cur);
    // 2x2x2 mean or mode levels fuse, up to three per launch, while every extent of a fused
    // level's input is >= 2 (window 2 on every axis); other levels run one launch each
    const bool fusable = ndim == 3 && factor[0] == 2 && factor[1] == 2 && factor[2] == 2 &&
                         zt::pyramid_fused_dtype(dtype, discrete != 0);
    auto level_shape = [&](int i) -> const int64_t* {  // shape of level i (0 = input)
        return i == 0 ? shape : shapes.data() + (size_t)(i - 1) * ndim;
    };
    for (int i = 0; i < n;) {
        int k = 0;
        while (fusable && k < 3 && i + k < n) {
            const int64_t* sh = level_shape(i + k);
            if (sh[0] < 2 || sh[1] < 2 || sh[2] < 2) break;
            ++k;
        }
        // the fused grid's y extent covers level-1 rows in fours: past 65535 workgroups (an
        // input y extent of ~524k) the levels run one launch each instead
        if (k >= 2 && !zt::pyramid_fused_grid_fits(level_shape(i + 1))) k = 0;
        if (k >= 2) {
            int64_t sh3[4][3] = {};
            for (int l = 0; l <= k; ++l) std::copy(level_shape(i + l), level_shape(i + l) + 3, sh3[l]);
            bool any = true;
            for (int d = 0; d < 3; ++d) any = any && sh3[1][d] > 0;
            if (any) {
                if (!src || !level_ptrs[i] || !level_ptrs[i + 1] || (k == 3 && !level_ptrs[i + 2]))
                    return fail(ZT_ERR_INVALID_PARAMETERS, "null level pointer");
                DeviceGuard g(ctx->device);
                if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev0, ctx->cur));
                hipError_t e = zt::launch_pyramid_fused(src, dtype, sh3, k, level_ptrs + i,
                                                       discrete != 0, ctx->cur);
                if (e != hipSuccess) return hip_fail(e, "fused pyramid launch");
                if (ctx->timed) ZT_HIP(hipEventRecord(ctx->ev1, ctx->cur));
            }
            src = level_ptrs[i + k - 1];
            std::copy(level_shape(i + k), level_shape(i + k) + ndim, cur);
            i += k;
            continue;
        }
        // level i+1 = downsample(level i), same dtype in/out (zarrs_ome.rs:211-234)
        int rc = zt_downsample_apply_ndarray(ctx, dtype, src, cur, ndim, factor, discrete, dtype,
                                             level_ptrs[i]);
        if (rc) return rc;
        src = level_ptrs[i];
        std::copy(shapes.data() + (size_t)i * ndim, shapes.data() + (size_t)(i + 1) * ndim, cur);
        ++i;
    }
    *levels_written = n;
    return ZT_OK;
}

// ---- synthetic inputs ------------------------------------------------------------------------

int zt_synth_step_noise_f32(zt_ctx* ctx, float* out, const int64_t* shape, int ndim,
                            const int64_t* global_shape, int64_t z0, uint64_t seed) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    const int64_t* gs = global_shape ? global_shape : shape;
    int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    int64_t plane = n / std::max<int64_t>(shape[0], 1);
    DeviceGuard g(ctx->device);
    hipError_t e = zt::launch_synth_step_noise_f32(out, n, plane, shape[ndim - 1], gs[ndim - 1],
                                                   z0, seed, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "synth launch");
    return ZT_OK;
}

int zt_synth_u16(zt_ctx* ctx, uint16_t* out, const int64_t* shape, int ndim,
                 const int64_t* global_shape, int64_t z0, uint64_t seed) {
    (void)global_shape;
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    int64_t n = numel(shape, ndim);
    if (n == 0) return ZT_OK;
    int64_t plane = n / std::max<int64_t>(shape[0], 1);
    DeviceGuard g(ctx->device);
    hipError_t e = zt::launch_synth_u16(out, n, plane, z0, seed, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "synth launch");
    return ZT_OK;
}

int zt_reencode_cast(zt_ctx* ctx, int dtype_in, const void* in, int dtype_out, void* out,
                     int64_t n) {
    if (int rc = begin_call(ctx)) return rc;
    if (zt::dtype_size(dtype_in) == 0 || zt::dtype_size(dtype_out) == 0)
        return fail(ZT_ERR_UNSUPPORTED_DATA_TYPE, "unsupported data type");
    if (n < 0) return fail(ZT_ERR_INVALID_PARAMETERS, "negative element count");
    if (n == 0) return ZT_OK;
    if (!in || !out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    hipError_t e = zt::launch_reencode_cast(in, dtype_in, out, dtype_out, n, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "reencode cast launch");
    return ZT_OK;
}

int zt_synth_box(zt_ctx* ctx, int kind, void* out, const int64_t* start, const int64_t* shape,
                 const int64_t* global_shape, int ndim, uint64_t seed) {
    if (int rc = begin_call(ctx)) return rc;
    if (int rc = check_shape(shape, ndim, "shape")) return rc;
    if (int rc = check_shape(global_shape, ndim, "global_shape")) return rc;
    if (!start) return fail(ZT_ERR_INVALID_PARAMETERS, "null start");
    if (kind != 0 && kind != 1) return fail(ZT_ERR_INVALID_PARAMETERS, "kind must be 0 or 1");
    for (int d = 0; d < ndim; ++d)
        if (start[d] < 0 || start[d] + shape[d] > global_shape[d])
            return fail(ZT_ERR_INVALID_PARAMETERS, "box outside the global shape on axis %d", d);
    if (numel(shape, ndim) == 0) return ZT_OK;
    if (!out) return fail(ZT_ERR_INVALID_PARAMETERS, "null data pointer");
    DeviceGuard g(ctx->device);
    hipError_t e = zt::launch_synth_box(out, kind, start, shape, global_shape, ndim, seed, ctx->cur);
    if (e != hipSuccess) return hip_fail(e, "synth launch");
    return ZT_OK;
}

}  // extern "C"
