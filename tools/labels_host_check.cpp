// labels_host_check.cpp — the host arithmetic of the label statistics and the label size filter
// (csrc/zt_labels_host.hpp): the columns and the size of the state, the label, element and origin
// limits and the bound that keeps a coordinate sum from wrapping, at their overflow edges: K at
// and above 2^31 - 2, 2^38 elements and one row more, origins next to INT64_MAX, n * (origin +
// extent) just under and at 2^64, zero extents next to huge ones, the filter's scratch.
// Host code only; build it with a sanitizer and run it on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/labels_host_check.cpp -o labels_host_check && ./labels_host_check
#include <cstdio>
#include <vector>

#include "../zarrs_tools_amd/csrc/zt_labels_host.hpp"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static zt::LblPlan plan_of(std::vector<int64_t> shape, std::vector<int64_t> origin, int64_t K,
                           bool intensity, int* status) {
    zt::LblPlan p;
    *status = zt::lbl_plan(shape.data(), origin.empty() ? nullptr : origin.data(),
                           (int)shape.size(), K, intensity, false, &p);
    return p;
}

int main() {
    int st = 0;
    // columns and words
    expect(zt::lbl_cols(3, false, false) == 10 && zt::lbl_cols(3, true, false) == 14, "columns");
    expect(zt::lbl_cols(8, true, false) == 29 && zt::lbl_cols(8, true, true) == 1, "columns, 8");
    zt::LblPlan p = plan_of({3, 5, 7}, {}, 4, false, &st);
    expect(st == zt::kLblOk && p.n == 105 && p.cols == 10 && p.state_words == 51 &&
               p.state_bytes == 408,
           "3x5x7, K = 4");
    p = plan_of({3, 5, 7}, {}, 0, true, &st);
    expect(st == zt::kLblOk && p.state_words == 15 && p.state_bytes == 120, "K = 0, intensity");
    // K at its limits
    p = plan_of({4}, {}, zt::kLblMaxLabels, true, &st);
    expect(st == zt::kLblOk && p.state_words == 8ull * 0x7FFFFFFFull + 1, "K = 2^31 - 2");
    plan_of({4}, {}, zt::kLblMaxLabels + 1, false, &st);
    expect(st == zt::kLblBadLabels, "K = 2^31 - 1");
    plan_of({4}, {}, -1, false, &st);
    expect(st == zt::kLblBadLabels, "K = -1");
    plan_of({4}, {}, INT64_MAX, false, &st);
    expect(st == zt::kLblBadLabels, "K = INT64_MAX");
    plan_of({4}, {}, INT64_MIN, false, &st);
    expect(st == zt::kLblBadLabels, "K = INT64_MIN");
    p = plan_of({1, 1, 1, 1, 1, 1, 1, 1}, {}, zt::kLblMaxLabels, true, &st);
    expect(st == zt::kLblOk && p.state_bytes == 8 * (29ull * 0x7FFFFFFFull + 1), "8 axes, largest K");
    // elements
    p = plan_of({1 << 13, 1 << 13, 1 << 12}, {}, 1, false, &st);
    expect(st == zt::kLblOk && p.n == zt::kLblMaxElems, "2^38 elements");
    plan_of({1 << 13, 1 << 13, (1 << 12) + 1}, {}, 1, false, &st);
    expect(st == zt::kLblTooManyElems, "2^38 + 2^26 elements");
    plan_of({INT64_MAX, INT64_MAX}, {}, 1, false, &st);
    expect(st == zt::kLblTooManyElems, "a product that is no int64");
    plan_of({2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647,
             2147483647}, {}, 1, false, &st);
    expect(st == zt::kLblTooManyElems, "eight extents of 2^31 - 1");
    // origins
    plan_of({4, 4}, {0, -1}, 1, false, &st);
    expect(st == zt::kLblBadOrigin, "origin -1");
    plan_of({4, 4}, {INT64_MIN, 0}, 1, false, &st);
    expect(st == zt::kLblBadOrigin, "origin INT64_MIN");
    plan_of({4, 4}, {0, INT64_MAX - 3}, 1, false, &st);
    expect(st == zt::kLblBadOrigin, "origin + extent = 2^63");
    p = plan_of({1, 1}, {0, INT64_MAX - 1}, 1, false, &st);
    expect(st == zt::kLblOk && p.n == 1, "one element at INT64_MAX - 1");
    // n * (largest origin + extent): 2^64 - 2^2 fits, 2^64 does not
    p = plan_of({4}, {((int64_t)1 << 62) - 5}, 1, false, &st);
    expect(st == zt::kLblOk && p.n == 4, "4 * (2^62 - 1)");
    plan_of({4}, {((int64_t)1 << 62) - 4}, 1, false, &st);
    expect(st == zt::kLblSumWraps, "4 * 2^62");
    plan_of({2, 2}, {0, INT64_MAX - 2}, 1, false, &st);
    expect(st == zt::kLblSumWraps, "4 * (2^63 - 1)");
    p = plan_of({1 << 13, 1 << 13, 1 << 12}, {0, 0, (1 << 26) - (1 << 12) - 1}, 1, false, &st);
    expect(st == zt::kLblOk, "2^38 * (2^26 - 1)");
    plan_of({1 << 13, 1 << 13, 1 << 12}, {(1 << 26) - (1 << 13), 0, 0}, 1, false, &st);
    expect(st == zt::kLblSumWraps, "2^38 * 2^26");
    // zero extents: no elements, whatever stands next to them (origins are still checked)
    p = plan_of({5, 0, 7}, {}, 3, true, &st);
    expect(st == zt::kLblOk && p.n == 0 && p.state_words == 57, "zero extent");
    p = plan_of({0, (int64_t)1 << 40}, {}, 3, false, &st);
    expect(st == zt::kLblOk && p.n == 0, "zero extent next to a huge one");
    p = plan_of({0, INT64_MAX}, {}, 3, false, &st);
    expect(st == zt::kLblOk && p.n == 0, "zero extent next to INT64_MAX");
    plan_of({0, 4}, {-1, 0}, 3, false, &st);
    expect(st == zt::kLblBadOrigin, "zero extent, origin -1");
    // the size filter's scratch: counts (K + 2 words), remap (4 (K + 1), padded to 8), two words
    uint64_t b = 0;
    expect(zt::lbl_filter_scratch(0, &b) == zt::kLblOk && b == 16 + 8 + 16, "scratch, K = 0");
    expect(zt::lbl_filter_scratch(1, &b) == zt::kLblOk && b == 24 + 8 + 16, "scratch, K = 1");
    expect(zt::lbl_filter_scratch(2, &b) == zt::kLblOk && b == 32 + 16 + 16, "scratch, K = 2");
    expect(zt::lbl_filter_scratch(zt::kLblMaxLabels, &b) == zt::kLblOk &&
               b == 8ull * 0x80000000ull + 4ull * 0x7FFFFFFFull + 4 + 16,
           "scratch, largest K");
    expect(zt::lbl_filter_scratch(zt::kLblMaxLabels + 1, &b) == zt::kLblBadLabels, "scratch, K + 1");

    if (failures) return 1;
    std::printf("labels_host_check ok\n");
    return 0;
}
