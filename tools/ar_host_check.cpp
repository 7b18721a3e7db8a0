// ar_host_check.cpp — the host half of the arithmetic store path's second input (run_pipeline's
// in2, csrc/host/zt_store.cpp): for every chunk row of a first array's grid, the chunks of a
// second array with another chunk grid (taller than the rows and not dividing them; once plain,
// once sharded and gzip compressed; its last chunk row missing, so it reads as the fill value)
// are decoded with Array::read_chunk into a row buffer of the first array's row shape, exactly as
// submit_decode does, and the buffer is compared with the array. The planes of the last row that
// lie beyond the array must stay untouched. Host code only; build it with a sanitizer and run it
// on the CPU:
//   hipcc -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined \
//       tools/ar_host_check.cpp zarrs_tools_amd/csrc/host/zt_zarr.cpp -o ar_host_check \
//       -fsanitize=address,undefined -lz -ldl -lpthread && ./ar_host_check
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../zarrs_tools_amd/csrc/host/zt_zarr.hpp"

using zt::zarr::Array;

static const int64_t kShape[3] = {37, 50, 70};
static const int64_t kRow = 16;  // the first array's chunk extent along axis 0
static const float kFill = -2.5f, kSentinel = 12345.0f;

static float value_at(int64_t z, int64_t y, int64_t x) {
    return (float)((z * 131 + y * 17 + x * 3) % 1000) * 0.25f;
}

static long check(const std::string& path, const char* codecs) {
    const std::vector<int64_t> shape(kShape, kShape + 3), chunk{24, 50, 35};
    Array a = Array::create(path, 11 /* float32 */, shape, chunk, zt::json::parse(codecs),
                            zt::json::parse("-2.5"));
    a.store_metadata();
    const int64_t plane = kShape[1] * kShape[2];
    std::vector<float> whole((size_t)(kShape[0] * plane));
    for (int64_t z = 0; z < kShape[0]; ++z)
        for (int64_t y = 0; y < kShape[1]; ++y)
            for (int64_t x = 0; x < kShape[2]; ++x)
                whole[(size_t)(z * plane + y * kShape[2] + x)] = value_at(z, y, x);
    const int64_t origin0[3] = {0, 0, 0}, st[3] = {plane, kShape[2], 1};
    for (int64_t cx = 0; cx < 2; ++cx) {  // the first chunk row only: the second stays missing
        const int64_t idx[3] = {0, 0, cx};
        a.write_chunk(idx, reinterpret_cast<const uint8_t*>(whole.data()), origin0, kShape, st);
    }
    Array b = Array::open(path);
    long checked = 0;
    const int64_t cz2 = b.chunk_shape[0], rows = (kShape[0] + kRow - 1) / kRow;
    const int64_t row_shape[3] = {kRow, kShape[1], kShape[2]};
    for (int64_t j = 0; j < rows; ++j) {
        std::vector<float> buf((size_t)(kRow * plane), kSentinel);
        const int64_t origin[3] = {j * kRow, 0, 0};
        const int64_t r0 = j * kRow / cz2;
        const int64_t r1 = (std::min((j + 1) * kRow, kShape[0]) + cz2 - 1) / cz2;
        for (int64_t r = r0; r < r1; ++r)
            for (int64_t cx = 0; cx < 2; ++cx) {
                const int64_t idx[3] = {r, 0, cx};
                b.read_chunk(idx, reinterpret_cast<uint8_t*>(buf.data()), origin, row_shape, st);
            }
        for (int64_t p = 0; p < kRow; ++p)
            for (int64_t i = 0; i < plane; ++i) {
                const int64_t z = j * kRow + p;
                const float want = z >= kShape[0] ? kSentinel
                                   : z >= cz2     ? kFill
                                                  : whole[(size_t)(z * plane + i)];
                if (buf[(size_t)(p * plane + i)] != want) {
                    std::printf("FAIL %s row %lld plane %lld element %lld: %g, expected %g\n",
                                path.c_str(), (long long)j, (long long)p, (long long)i,
                                buf[(size_t)(p * plane + i)], want);
                    std::exit(1);
                }
                ++checked;
            }
    }
    return checked;
}

int main() {
    char tmpl[] = "/tmp/ar_host_check_XXXXXX";
    const char* dir = mkdtemp(tmpl);
    if (!dir) {
        std::perror("mkdtemp");
        return 1;
    }
    long n = 0;
    try {
        n += check(std::string(dir) + "/plain",
                   "[{\"name\":\"bytes\",\"configuration\":{\"endian\":\"little\"}}]");
        n += check(std::string(dir) + "/sharded",
                   "[{\"name\":\"sharding_indexed\",\"configuration\":{\"chunk_shape\":[12,25,35],"
                   "\"codecs\":[{\"name\":\"bytes\",\"configuration\":{\"endian\":\"little\"}},"
                   "{\"name\":\"gzip\",\"configuration\":{\"level\":1}}],"
                   "\"index_codecs\":[{\"name\":\"bytes\",\"configuration\":{\"endian\":\"little\"}},"
                   "{\"name\":\"crc32c\"}],\"index_location\":\"end\"}}]");
    } catch (const std::exception& e) {
        std::printf("FAIL %s\n", e.what());
        return 1;
    }
    std::string rm = std::string("rm -rf ") + dir;
    if (std::system(rm.c_str()) != 0) return 1;
    std::printf("ok: %ld elements checked\n", n);
    return 0;
}
