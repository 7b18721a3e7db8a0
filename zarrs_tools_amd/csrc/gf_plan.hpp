// gf_plan.hpp — the launch decision of the fused 3-D guided filter (gf_fused.hpp), kept free of
// HIP headers so the host unit test (tests/test_gf_plan.py) compiles it with g++ alone. Every
// predicate of the decision lives here once: the tile shape per radius, the quad-aligned
// geometry test (one mode-1 grid, else mode 0 + mode 2), the interior tile range and the z-march
// length. run_fused3 (zt_api.hip) makes the plan, launch_fused_cfg (gf_fused.hpp) follows it.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace zt {

constexpr int kFusedTileX = 64;  // output tile width of the fused kernel (GFConfig::TX)
// output tile height of the fused kernel for a radius (the TY of GFConfig in gf_fused_r<R>.hip)
constexpr int fused_tile_y(int radius) { return radius <= 4 ? 32 : 16; }

inline long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// Interior tile range along one axis: tiles t with origin o0 + t*T such that the whole E2 apron
// [o0 + t*T - 2R, o0 + t*T + T + 2R + slack) is inside [0, n) and the output tile inside
// [o0, o_end). Returns [lo, hi) (empty when lo >= hi).
inline void interior_tiles(long long o0, long long o_end, long long n, int T, int R, int slack,
                           int ntiles, int& lo, int& hi) {
    long long l = ceil_div(2LL * R - o0, T);
    long long h = floor_div(std::min(n - 2LL * R - slack, o_end) - T - o0, T) + 1;
    l = std::max(l, 0LL);
    h = std::min(h, (long long)ntiles);
    if (h < l) h = l;
    lo = (int)l;
    hi = (int)h;
}

// Choose the z-march length for a fused launch: whole chunk depths when there is enough
// parallelism, shorter segments for a single small block. Segments are a free choice (windows
// are clamped at the array, not the segment), so large launches march two chunk depths while
// they keep >= 4096 workgroups (16 per CU): each segment re-fills its z-windows over 2r + 1
// warm-up slices and pads its steps to a multiple of 2r + 1 (2048^3 r=4: 31.4 -> 30.6 ms;
// 384- and 1024-slice segments measured slower, tools/timek.sh; profiles/r02_ab_harness.txt).
inline int choose_zseg(int onz, int tiles, int radius, int chunk_depth) {
    const int target_wg = 1024;
    int zseg = chunk_depth > 0 ? std::min(chunk_depth, onz) : onz;
    if (zseg <= 0) zseg = 1;
    if (chunk_depth > 0 && radius <= 2) {
        // short windows (5-slice warm-up): up to 4 chunk depths while >= 512 workgroups (2 per CU)
        // remain (1024^3 r=2: 3.46 -> 3.33 ms for one 1024-slice segment per tile)
        for (int m = 4; m >= 2; m /= 2)
            if ((int64_t)m * chunk_depth <= onz &&
                (int64_t)tiles * ((onz + m * chunk_depth - 1) / (m * chunk_depth)) >= 512) {
                zseg = m * chunk_depth;
                break;
            }
    } else if (chunk_depth > 0 && 2LL * chunk_depth <= onz &&
               (int64_t)tiles * ((onz + 2 * chunk_depth - 1) / (2 * chunk_depth)) >= 4096) {
        zseg = 2 * chunk_depth;
    }
    int64_t wg = (int64_t)tiles * ((onz + zseg - 1) / zseg);
    if (wg < target_wg && chunk_depth <= 0) {
        int nseg = (target_wg + tiles - 1) / std::max(tiles, 1);
        int minseg = std::max(8, 4 * radius);
        zseg = std::max(minseg, (onz + nseg - 1) / nseg);
        zseg = std::min(zseg, onz);
    }
    return zseg;
}

// Geometry of one fused launch, in elements (GFParams' fields of the same names).
struct FusedGeom {
    int ny, nx;                // domain extent in y and x
    int oy0, ox0;              // output box origin
    int onz, ony, onx;         // output box extent
    int64_t in_sz, in_sy;      // input plane / row stride
    int64_t out_sz, out_sy;    // output plane / row stride
};

// Quad-aligned geometry: every 4-element quad of a global access starts at a multiple of 4
// elements (the E2 apron at x0 - 2R, the output tile at x0; the domain / output box widths and
// every stride multiples of 4, both base addresses on a quad), so no quad straddles a boundary
// and every tile can take the unmasked mode 1.
inline bool fused_quad_ok(const FusedGeom& g, int R, int esz_in, int esz_out, uintptr_t in,
                          uintptr_t out) {
    return (g.ox0 % 4 == 0) && (R % 2 == 0) && (g.nx % 4 == 0) && (g.onx % 4 == 0) &&
           (g.in_sy % 4 == 0) && (g.in_sz % 4 == 0) && (g.out_sy % 4 == 0) &&
           (g.out_sz % 4 == 0) && (in % (4 * (uintptr_t)esz_in) == 0) &&
           (out % (4 * (uintptr_t)esz_out) == 0);
}

// What a fused launch does. mode1: one grid of tiles_x * tiles_y * nseg workgroups in mode 1 (the
// interior range is then empty). Otherwise the tiles [itx0, itx1) x [ity0, ity1) run in mode 0
// (a grid of that many tiles * nseg, none when the range is empty) and, when any tile is left,
// mode 2 over the whole tile grid (its interior workgroups return at once).
struct FusedPlan {
    bool mode1;
    int tiles_x, tiles_y;
    int itx0, itx1, ity0, ity1;
    int zseg, nseg;
};

// chunk_depth > 0: the z-march follows the chunk depth; 0: free choice (a single block).
// zseg_fixed > 0 overrides the march length (the timing tools sweep it).
inline FusedPlan plan_fused(const FusedGeom& g, int R, int esz_in, int esz_out, uintptr_t in,
                            uintptr_t out, int chunk_depth, int zseg_fixed = 0) {
    FusedPlan pl{};
    const int TX = kFusedTileX, TY = fused_tile_y(R);
    pl.tiles_x = (g.onx + TX - 1) / TX;
    pl.tiles_y = (g.ony + TY - 1) / TY;
    const int tiles = (int)((int64_t)pl.tiles_x * pl.tiles_y);
    pl.zseg = zseg_fixed > 0 ? zseg_fixed : choose_zseg(g.onz, tiles, R, chunk_depth);
    pl.nseg = (g.onz + pl.zseg - 1) / pl.zseg;
    pl.mode1 = fused_quad_ok(g, R, esz_in, esz_out, in, out);
    if (!pl.mode1) {
        interior_tiles(g.ox0, (long long)g.ox0 + g.onx, g.nx, TX, R, 0, pl.tiles_x, pl.itx0,
                       pl.itx1);
        interior_tiles(g.oy0, (long long)g.oy0 + g.ony, g.ny, TY, R, 0, pl.tiles_y, pl.ity0,
                       pl.ity1);
    }
    return pl;
}

}  // namespace zt
