// zt_occupancy.hpp — the geometry of the chunk-occupancy pass (occupancy.hip): a contiguous
// C-order box seen as rows of `row` elements, and where a row lies in the grid of cells. The row
// bookkeeping is plain integer code shared by the kernel and by a host check (tools/
// occ_host_check.cpp), which walks the same functions over a box and tests every cell index
// against its bound.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZT_OCC_HD __host__ __device__ __forceinline__
#else
#define ZT_OCC_HD inline
#endif

namespace zt {

constexpr int kOccOuter = 7;  // axes in front of the row axis (kMaxDims - 1), right-aligned

// The box after occupancy_geom() merged what can be merged: rows of `row` elements whose cells
// are `cell_x` wide and consecutive in the map; outer axis slot kOccOuter-1 is the axis in front
// of the row axis, unused leading slots have extent 1, cell 1 and stride 0.
struct OccGeom {
    int64_t n;       // elements of the box
    int64_t cells;   // cells of the map
    int64_t row, cell_x;
    int64_t shape[kOccOuter], cell[kOccOuter];
    int64_t gstride[kOccOuter];  // map stride of one cell step along the axis
    int64_t wrap[kOccOuter];     // (cells along the axis - 1) * gstride
};

// shape / cell_shape (ndim <= 8 extents, all >= 1) -> g. Cells larger than the box are clamped;
// an axis with one cell is merged into the axis in front of it (the cell index does not change),
// so a box whose last axes are not cut has long rows.
inline void occupancy_geom(const int64_t* shape, const int64_t* cell_shape, int ndim, OccGeom* g) {
    int64_t sh[8], cs[8], gs[8], gr[8];
    int nd = ndim;
    int64_t stride = 1, n = 1;
    for (int d = nd - 1; d >= 0; --d) {
        sh[d] = shape[d];
        cs[d] = cell_shape[d] < shape[d] ? cell_shape[d] : shape[d];
        gr[d] = (sh[d] + cs[d] - 1) / cs[d];
        gs[d] = stride;
        stride *= gr[d];
        n *= sh[d];
    }
    g->n = n;
    g->cells = stride;
    for (int d = nd - 1; d >= 1; --d) {
        if (gr[d] != 1) continue;
        sh[d - 1] *= sh[d];
        cs[d - 1] *= sh[d];
        for (int e = d; e + 1 < nd; ++e) {
            sh[e] = sh[e + 1]; cs[e] = cs[e + 1]; gs[e] = gs[e + 1]; gr[e] = gr[e + 1];
        }
        --nd;
    }
    g->row = sh[nd - 1];
    g->cell_x = cs[nd - 1];
    for (int k = 0; k < kOccOuter; ++k) {
        const int d = nd - 2 - (kOccOuter - 1 - k);
        g->shape[k] = d >= 0 ? sh[d] : 1;
        g->cell[k] = d >= 0 ? cs[d] : 1;
        g->gstride[k] = d >= 0 ? gs[d] : 0;
        g->wrap[k] = d >= 0 ? (gr[d] - 1) * gs[d] : 0;
    }
}

// Where a row lies: x = the position in the row, c / m = the row's coordinate and its offset in
// the cell along every outer axis, rowcell = the map index of the row's first cell.
struct OccRow {
    int64_t x, rowcell;
    int64_t c[kOccOuter], m[kOccOuter];

    // the row of element e (divisions: once per wave, and for head and tail elements)
    ZT_OCC_HD void init(const OccGeom& g, int64_t e) {
        int64_t r = e / g.row;
        x = e - r * g.row;
        rowcell = 0;
#pragma unroll
        for (int d = kOccOuter - 1; d >= 0; --d) {
            const int64_t q = r / g.shape[d], cd = r - q * g.shape[d];
            r = q;
            const int64_t k = cd / g.cell[d];
            c[d] = cd;
            m[d] = cd - k * g.cell[d];
            rowcell += k * g.gstride[d];
        }
    }
    // the next row (an odometer: no division); after the last row, the first again
    ZT_OCC_HD void next_row(const OccGeom& g) {
        bool carry = true;
#pragma unroll
        for (int d = kOccOuter - 1; d >= 0; --d) {
            if (!carry) continue;
            if (++c[d] < g.shape[d]) {
                carry = false;
                if (++m[d] == g.cell[d]) {
                    m[d] = 0;
                    rowcell += g.gstride[d];
                }
            } else {
                rowcell -= g.wrap[d];
                c[d] = 0;
                m[d] = 0;
            }
        }
    }
    ZT_OCC_HD void advance(const OccGeom& g, int64_t count) {
        x += count;
        while (x >= g.row) {
            x -= g.row;
            next_row(g);
        }
    }
};

// the map index of element e, from scratch
ZT_OCC_HD int64_t occupancy_cell_of(const OccGeom& g, int64_t e) {
    OccRow r;
    r.init(g, e);
    return r.rowcell + r.x / g.cell_x;
}

}  // namespace zt
