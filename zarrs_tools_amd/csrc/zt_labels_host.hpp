// zt_labels_host.hpp — the host-side arithmetic of the label statistics: the
// columns of the state, its size, and the limits that keep every device sum from wrapping. Plain
// C++ with no HIP in it, so tools/labels_host_check.cpp compiles it for the CPU under sanitizers.
#pragma once

#include <stdint.h>

namespace zt {

constexpr int kLblMaxDims = 8;                        // ZT_MAX_DIMS
constexpr int64_t kLblMaxLabels = 0x7FFFFFFEll;       // K <= 2^31 - 2
constexpr int64_t kLblMaxElems = (int64_t)1 << 38;    // as the labelling

enum LblStatus : int {
    kLblOk = 0,
    kLblBadLabels = 1,      // K < 0 or K > 2^31 - 2
    kLblBadOrigin = 2,      // a negative origin, or origin + extent is no int64_t
    kLblTooManyElems = 3,   // more than 2^38 elements in the box
    kLblSumWraps = 4,       // n * (largest origin + extent) >= 2^64: a coordinate sum could wrap
    kLblStateTooLarge = 5,  // the state's byte count is no uint64_t
};

// The state: (K + 1) rows of `cols` u64 columns, struct-of-arrays (column c of label l is word
// c * (K + 1) + l), then one word that counts the elements outside [0, K].
//   column 0                 count
//   columns 1 + 3a .. 3 + 3a smallest, largest (inclusive) and summed coordinate on axis a
//   with intensity, after the axes: smallest key, largest key, sum lo, sum hi
// count_only: column 0 alone (the label size filter).
inline int lbl_cols(int ndim, bool intensity, bool count_only) {
    return count_only ? 1 : 1 + 3 * ndim + (intensity ? 4 : 0);
}

struct LblPlan {
    int64_t n = 0;             // elements of the box; 0 when an extent is 0
    int cols = 0;
    uint64_t state_words = 0;  // cols * (K + 1) + 1
    uint64_t state_bytes = 0;
};

// The state of K labels over `ndim` axes (ndim in [1, kLblMaxDims]).
inline int lbl_state(int ndim, int64_t n_labels, bool intensity, bool count_only, LblPlan* plan) {
    if (n_labels < 0 || n_labels > kLblMaxLabels) return kLblBadLabels;
    LblPlan p;
    p.cols = lbl_cols(ndim, intensity, count_only);
    uint64_t words, bytes;
    if (__builtin_mul_overflow((uint64_t)p.cols, (uint64_t)n_labels + 1, &words) ||
        __builtin_add_overflow(words, (uint64_t)1, &words) ||
        __builtin_mul_overflow(words, (uint64_t)8, &bytes))
        return kLblStateTooLarge;
    p.state_words = words;
    p.state_bytes = bytes;
    *plan = p;
    return kLblOk;
}

// The state and the limits of one accumulate over the box `shape` (every extent >= 0) that lies
// at `origin` (NULL = zeros) of the whole array. Every product and sum is checked.
inline int lbl_plan(const int64_t* shape, const int64_t* origin, int ndim, int64_t n_labels,
                    bool intensity, bool count_only, LblPlan* plan) {
    LblPlan p;
    if (int st = lbl_state(ndim, n_labels, intensity, count_only, &p)) return st;
    int64_t max_end = 0;
    bool empty = false;
    for (int a = 0; a < ndim; ++a) {
        const int64_t o = origin ? origin[a] : 0;
        int64_t end;
        if (o < 0 || __builtin_add_overflow(o, shape[a], &end)) return kLblBadOrigin;
        if (end > max_end) max_end = end;
        if (shape[a] == 0) empty = true;
    }
    if (!empty) {
        int64_t n = 1;
        for (int a = 0; a < ndim; ++a)
            if (__builtin_mul_overflow(n, shape[a], &n) || n > kLblMaxElems)
                return kLblTooManyElems;
        uint64_t worst;  // n elements, each coordinate below max_end
        if (__builtin_mul_overflow((uint64_t)n, (uint64_t)max_end, &worst)) return kLblSumWraps;
        p.n = n;
    }
    *plan = p;
    return kLblOk;
}

// The label size filter's scratch: the count-only state, then K + 1 remap entries (uint32_t,
// padded to 8 bytes) and two words: the kept count K' and the largest label kept.
inline int lbl_filter_scratch(int64_t n_labels, uint64_t* bytes) {
    LblPlan p;
    if (int st = lbl_state(1, n_labels, false, true, &p)) return st;
    const uint64_t remap = (((uint64_t)n_labels + 1) * 4 + 7) & ~(uint64_t)7;
    *bytes = p.state_bytes + remap + 16;  // K <= 2^31 - 2: far from wrapping
    return kLblOk;
}

}  // namespace zt
