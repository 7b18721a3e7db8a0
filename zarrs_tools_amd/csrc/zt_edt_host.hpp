// zt_edt_host.hpp — the host-side arithmetic of the distance transform: the
// bound B on the squared distance, the work width it selects, the limits and the memory formula.
// Plain C++ with no HIP in it, so tools/edt_host_check.cpp compiles it for the CPU under
// sanitizers.
#pragma once

#include <stdint.h>

namespace zt {

constexpr int kEdtMaxDims = 8;                        // ZT_MAX_DIMS
constexpr int64_t kEdtMaxElems = (int64_t)1 << 38;    // as the labelling
constexpr int64_t kEdtMaxExtent = (int64_t)1 << 31;   // every extent is below this
constexpr uint64_t kEdtBoundLimit = 1ull << 62;       // B >= this: InvalidParameters
constexpr uint64_t kEdtBound32 = 0xFFFFFFFFull;       // B < this: uint32_t work elements

enum EdtStatus : int {
    kEdtOk = 0,
    kEdtBadSpacing = 1,   // a spacing below 1
    kEdtBoundTooLarge = 2,  // B >= 2^62 (or not even a uint64_t)
    kEdtTooManyElems = 3,
    kEdtExtentTooLarge = 4,
};

struct EdtPlan {
    int64_t n = 0;                 // elements; 0 when an extent is 0
    uint64_t bound = 0;            // B = sum of spacing_a^2 * (n_a - 1)^2
    uint64_t weight[kEdtMaxDims];  // spacing_a^2; 0 for an axis of extent <= 1 (never used)
    bool work64 = false;           // from B alone; the caller ORs the ZT_EDT_WORK64 switch in
};

// Fills `plan` for `shape` (every extent >= 0, ndim in [1, kEdtMaxDims]) and `spacing` (NULL =
// ones). Nothing here overflows: every product and sum is checked, and an overflow is
// kEdtBoundTooLarge since such a B is certainly >= 2^62. A zero extent gives n = 0, kEdtOk after
// the spacing itself was checked.
inline int edt_plan(const int64_t* shape, const int64_t* spacing, int ndim, EdtPlan* plan) {
    EdtPlan p;
    for (int a = 0; a < kEdtMaxDims; ++a) p.weight[a] = 0;
    for (int a = 0; a < ndim; ++a)
        if (spacing && spacing[a] < 1) return kEdtBadSpacing;
    int64_t n = 1;
    for (int a = 0; a < ndim; ++a) {
        if (shape[a] == 0) {
            *plan = p;
            return kEdtOk;
        }
    }
    for (int a = 0; a < ndim; ++a) {
        if (shape[a] >= kEdtMaxExtent) return kEdtExtentTooLarge;
        if (__builtin_mul_overflow(n, shape[a], &n) || n > kEdtMaxElems) return kEdtTooManyElems;
    }
    uint64_t bound = 0;
    for (int a = 0; a < ndim; ++a) {
        if (shape[a] <= 1) continue;  // no distance along this axis, whatever its spacing
        const uint64_t s = spacing ? (uint64_t)spacing[a] : 1, e = (uint64_t)shape[a] - 1;
        uint64_t w, term;
        if (__builtin_mul_overflow(s, s, &w) || __builtin_mul_overflow(w, e * e, &term) ||
            __builtin_add_overflow(bound, term, &bound) || bound >= kEdtBoundLimit)
            return kEdtBoundTooLarge;
        p.weight[a] = w;
    }
    p.n = n;
    p.bound = bound;
    p.work64 = bound >= kEdtBound32;
    *plan = p;
    return kEdtOk;
}

// Scratch of one call: two work arrays of n elements (an axis pass reads one and writes the
// other, so the value at a parabola's apex is still there after the line's output was written) and
// the per-lane stacks laid out like the array, one 8-byte slot per element: the apex position and
// the breakpoint (4 bytes each).
inline uint64_t edt_scratch_bytes(int64_t n, bool work64) {
    return (uint64_t)n * (2 * (work64 ? 8u : 4u) + 8u);
}

}  // namespace zt
