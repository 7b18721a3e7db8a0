// edt_host_check.cpp — the host arithmetic of the distance transform (csrc/zt_edt_host.hpp): the
// bound B = sum of spacing^2 * (extent - 1)^2, the work width it selects, the limits and the
// scratch formula, at their overflow edges: B just under and at 2^32 - 1 and 2^62, a spacing of
// 2^31 - 1, spacings whose square is no uint64_t, the element and extent limits, zero extents.
// Host code only; build it with a sanitizer and run it on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/edt_host_check.cpp -o edt_host_check && ./edt_host_check
#include <cstdio>
#include <vector>

#include "../zarrs_tools_amd/csrc/zt_edt_host.hpp"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static zt::EdtPlan plan_of(std::vector<int64_t> shape, std::vector<int64_t> spacing, int* status) {
    zt::EdtPlan p;
    *status = zt::edt_plan(shape.data(), spacing.empty() ? nullptr : spacing.data(),
                           (int)shape.size(), &p);
    return p;
}

int main() {
    int st = 0;
    zt::EdtPlan p = plan_of({3, 5, 7}, {}, &st);
    expect(st == zt::kEdtOk && p.n == 105 && p.bound == 4 + 16 + 36 && !p.work64, "3x5x7, ones");
    expect(p.weight[0] == 1 && p.weight[1] == 1 && p.weight[2] == 1, "weights of ones");
    p = plan_of({3, 5, 7}, {70000, 1, 1}, &st);
    expect(st == zt::kEdtOk && p.bound == 4ull * 70000 * 70000 + 52 && p.work64, "70000 on z");
    expect(p.weight[0] == 70000ull * 70000, "weight of 70000");

    // 65535^2 + 362^2 + 5^2 = 2^32 - 2: the last B with 32-bit work; one more is the sentinel
    p = plan_of({2, 2, 2}, {65535, 362, 5}, &st);
    expect(st == zt::kEdtOk && p.bound == 0xFFFFFFFEull && !p.work64, "B = 2^32 - 2");
    p = plan_of({2, 2, 2, 2}, {65535, 362, 5, 1}, &st);
    expect(st == zt::kEdtOk && p.bound == 0xFFFFFFFFull && p.work64, "B = 2^32 - 1");
    p = plan_of({65536}, {}, &st);
    expect(st == zt::kEdtOk && !p.work64, "extent 65536");
    p = plan_of({65537}, {}, &st);
    expect(st == zt::kEdtOk && p.bound == 1ull << 32 && p.work64, "extent 65537");

    // spacing 2^31 - 1: its square is below 2^62 on an extent of 2 and four times that on 3
    const int64_t big = 0x7FFFFFFFll;
    p = plan_of({2}, {big}, &st);
    expect(st == zt::kEdtOk && p.bound == (uint64_t)big * big && p.bound < zt::kEdtBoundLimit,
           "spacing 2^31 - 1, extent 2");
    plan_of({3}, {big}, &st);
    expect(st == zt::kEdtBoundTooLarge, "spacing 2^31 - 1, extent 3");
    // B just under 2^62: (2^31 - 1)^2 = 2^62 - 2^32 + 1, and 2^32 - 2 as above ... and one more
    p = plan_of({2, 2, 2, 2}, {big, 65535, 362, 5}, &st);
    expect(st == zt::kEdtOk && p.bound == zt::kEdtBoundLimit - 1 && p.work64, "B = 2^62 - 1");
    plan_of({2, 2, 2, 2, 2}, {big, 65535, 362, 5, 1}, &st);
    expect(st == zt::kEdtBoundTooLarge, "B = 2^62, five axes");
    plan_of({2}, {(int64_t)1 << 31}, &st);
    expect(st == zt::kEdtBoundTooLarge, "B = 2^62");
    // squares and products that are no uint64_t
    plan_of({2}, {(int64_t)1 << 33}, &st);
    expect(st == zt::kEdtBoundTooLarge, "spacing 2^33");
    plan_of({2, 2}, {1, INT64_MAX}, &st);
    expect(st == zt::kEdtBoundTooLarge, "spacing INT64_MAX");
    plan_of({2147483647}, {3}, &st);
    expect(st == zt::kEdtBoundTooLarge, "extent 2^31 - 1, spacing 3");
    p = plan_of({2147483647}, {1}, &st);
    expect(st == zt::kEdtOk && p.bound == (uint64_t)(big - 1) * (big - 1) && p.work64,
           "extent 2^31 - 1, spacing 1");
    // an axis of extent 1 has no distance, whatever its spacing
    p = plan_of({1, 9}, {INT64_MAX, 2}, &st);
    expect(st == zt::kEdtOk && p.bound == 4 * 64 && p.weight[0] == 0 && p.weight[1] == 4,
           "extent 1");
    // spacings below 1
    plan_of({4, 5}, {0, 1}, &st);
    expect(st == zt::kEdtBadSpacing, "spacing 0");
    plan_of({4, 5}, {1, -2}, &st);
    expect(st == zt::kEdtBadSpacing, "spacing -2");
    plan_of({4, 0}, {1, INT64_MIN}, &st);
    expect(st == zt::kEdtBadSpacing, "spacing INT64_MIN with a zero extent");
    // limits
    plan_of({(int64_t)1 << 31}, {}, &st);
    expect(st == zt::kEdtExtentTooLarge, "extent 2^31");
    plan_of({1 << 13, 1 << 13, (1 << 12) + 1}, {}, &st);
    expect(st == zt::kEdtTooManyElems, "2^38 + 2^26 elements");
    p = plan_of({1 << 13, 1 << 13, 1 << 12}, {}, &st);
    expect(st == zt::kEdtOk && p.n == zt::kEdtMaxElems, "2^38 elements");
    plan_of({2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647,
             2147483647}, {}, &st);
    expect(st == zt::kEdtTooManyElems, "eight extents of 2^31 - 1");
    // zero extents
    p = plan_of({5, 0, 7}, {}, &st);
    expect(st == zt::kEdtOk && p.n == 0 && p.bound == 0, "zero extent");
    p = plan_of({0, (int64_t)1 << 40}, {}, &st);
    expect(st == zt::kEdtOk && p.n == 0, "zero extent next to a huge one");
    // scratch: two work arrays and two 4-byte stacks
    expect(zt::edt_scratch_bytes(105, false) == 105 * 16, "scratch, 32 bits");
    expect(zt::edt_scratch_bytes(105, true) == 105 * 24, "scratch, 64 bits");
    expect(zt::edt_scratch_bytes(zt::kEdtMaxElems, true) == 24ull << 38, "scratch, 2^38 elements");

    if (failures) return 1;
    std::printf("edt_host_check ok\n");
    return 0;
}
