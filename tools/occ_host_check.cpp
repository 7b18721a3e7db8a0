// occ_host_check.cpp — a host walk of the chunk-occupancy kernel's indexing (csrc/occupancy.hip)
// through the functions it shares with the kernel (csrc/zt_occupancy.hpp): for random boxes, cell
// shapes, element sizes, alignments and wave counts, every wave steps through its chunks as the
// kernel does (a random mix of the "all fill" step and the row walk), and the cell the walk gives
// every element is compared with the cell of the element's unravelled coordinates and with the
// map's bound. Host code only; build it with a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I zarrs_tools_amd/csrc \
//       tools/occ_host_check.cpp -o occ_host_check && ./occ_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "zt_occupancy.hpp"

using zt::OccGeom;

static int64_t brute_cell(const int64_t* shape, const int64_t* cell, int nd, int64_t e) {
    int64_t idx[8], g[8];
    for (int d = nd - 1; d >= 0; --d) {
        idx[d] = e % shape[d];
        e /= shape[d];
        g[d] = (shape[d] + cell[d] - 1) / cell[d];
    }
    int64_t c = 0;
    for (int d = 0; d < nd; ++d) c = c * g[d] + idx[d] / cell[d];
    return c;
}

static long g_checked = 0;

static void check(const int64_t* shape, const int64_t* cell, int nd, int esz, int head_want,
                  int64_t waves, std::mt19937_64& rng) {
    OccGeom g;
    zt::occupancy_geom(shape, cell, nd, &g);
    const int per = 16 / esz;
    const int64_t chunk_vecs = 256;
    const int64_t head = head_want < g.n ? head_want : g.n;
    const int64_t nvec = (g.n - head) / per;
    const int64_t nchunks = (nvec + chunk_vecs - 1) / chunk_vecs;
    const int64_t per_wave = waves ? (nchunks + waves - 1) / waves : 0;
    std::vector<char> seen((size_t)g.n, 0);
    auto expect = [&](int64_t e, int64_t got) {
        const int64_t want = brute_cell(shape, cell, nd, e);
        if (got != want || got < 0 || got >= g.cells) {
            std::printf("FAIL element %lld: cell %lld, expected %lld of %lld\n", (long long)e,
                        (long long)got, (long long)want, (long long)g.cells);
            std::exit(1);
        }
        seen[(size_t)e] = 1;
        ++g_checked;
    };
    for (int64_t w = 0; w < waves; ++w) {
        int64_t ch = w * per_wave;
        const int64_t ch_end = ch + per_wave < nchunks ? ch + per_wave : nchunks;
        if (ch >= ch_end) continue;
        zt::OccRow st;
        bool placed = false;
        for (; ch < ch_end; ++ch) {
            const int64_t vbase = ch * chunk_vecs;
            const int64_t nv = nvec - vbase < chunk_vecs ? nvec - vbase : chunk_vecs;
            const int64_t ne = nv * per;
            if (placed && st.x + ne <= g.row) {  // the flags the kernel would read before a chunk
                const int64_t k0 = st.x / g.cell_x, k1 = (st.x + ne - 1) / g.cell_x;
                if (st.rowcell + k0 < 0 || st.rowcell + k1 >= g.cells) {
                    std::printf("FAIL flag range\n");
                    std::exit(1);
                }
            }
            if (rng() % 3 == 0) {  // "all fill": only the position moves
                for (int64_t i = 0; i < ne; ++i) seen[(size_t)(head + vbase * per + i)] = 1;
                if (rng() % 2 && placed) st.advance(g, ne);  // (all marked: the odometer)
                else if (placed && st.x + ne < g.row) st.x += ne;
                else placed = false;
                continue;
            }
            if (!placed) {
                st.init(g, head + vbase * per);
                placed = true;
            }
            int64_t off = 0;
            while (off < ne) {
                const int64_t len = ne - off < g.row - st.x ? ne - off : g.row - st.x;
                for (int64_t j = 0; j < nv; ++j) {
                    const int64_t e0 = j * per;
                    const int64_t a = e0 > off ? e0 : off;
                    const int64_t b = e0 + per < off + len ? e0 + per : off + len;
                    if (a >= b) continue;
                    const int64_t xe = st.x + (a - off);
                    int64_t k = xe / g.cell_x, m = xe - k * g.cell_x;
                    if (m + (b - a) <= g.cell_x) {  // one cell holds all of them
                        for (int64_t e = a; e < b; ++e) expect(head + vbase * per + e, st.rowcell + k);
                        continue;
                    }
                    for (int i = 0; i < per; ++i) {
                        if (e0 + i < a || e0 + i >= b) continue;
                        expect(head + vbase * per + e0 + i, st.rowcell + k);
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
    for (int64_t e = 0; e < head; ++e) expect(e, zt::occupancy_cell_of(g, e));
    for (int64_t e = head + nvec * per; e < g.n; ++e) expect(e, zt::occupancy_cell_of(g, e));
    for (int64_t e = 0; e < g.n; ++e)
        if (!seen[(size_t)e]) {
            std::printf("FAIL element %lld not visited\n", (long long)e);
            std::exit(1);
        }
}

int main() {
    std::mt19937_64 rng(12345);
    const int esizes[4] = {1, 2, 4, 8};
    for (int it = 0; it < 4000; ++it) {
        const int nd = 1 + (int)(rng() % 8);
        int64_t shape[8], cell[8], n = 1;
        for (int d = 0; d < nd; ++d) {
            const int64_t cap = nd == 1 ? 5000 : nd <= 3 ? 40 : 6;
            shape[d] = 1 + (int64_t)(rng() % cap);
            cell[d] = rng() % 4 == 0 ? shape[d] + (int64_t)(rng() % 3) : 1 + (int64_t)(rng() % shape[d]);
            n *= shape[d];
        }
        if (n > 200000) continue;
        const int esz = esizes[rng() % 4];
        const int head = (int)(rng() % (16 / esz));
        const int64_t waves = 1 + (int64_t)(rng() % 9);
        check(shape, cell, nd, esz, head, waves, rng);
    }
    // the cases of the GPU tests
    {
        const int64_t s[3] = {3, 5, 23}, c[3] = {2, 2, 5};
        for (int h = 0; h < 16; ++h) check(s, c, 3, 1, h, 4, rng);
    }
    std::printf("ok: %ld elements checked\n", g_checked);
    return 0;
}
