// C19. The exact, truncated Euclidean distance field of a box of voxels of the accumulated scene cloud, with the nearest row (a feature transform), its
// planar (x, y) form and the lookup of points in it (accum_field.hip; include/pcacc.h C19), as __host__ __device__ functions, so
// that the SAME code runs in the kernels and in a g++ build (tests/accum_field_host_driver.cpp) where every index is assert-checked before anything runs
// on a GPU.  Includes nothing of HIP.  Nothing of C4 - C17 is restated: accum_unkey, accum_point, accn_in_range, accc_map_row, accc_column_key are called.
//
//   box       integer origin (x0, y0, z0), each |.| <= 2^31, shape (nx, ny, nz), each >= 1; planar: the field is over (x, y) only, nz_out = 1, else
//             nz_out = nz; cells = nx ny nz_out <= 2^28.  Cell (i, j, k) is element (i ny + j) nz_out + k and stands for voxel (x0 + i, y0 + j, z0 + k).
//   sites     the rows of extract() under the filter (rows[kept] of pass 1 of C5; j denotes such a row) whose voxel lies inside the box.  Indices are
//             subtracted in int64; a cell outside [-2^20, 2^20) never holds a site and no key is formed for it: keys are only decoded.  Keys are
//             unique, so a cell has at most one site.  Planar: a site is any kept voxel with z in [z0, z0 + nz); rows ascend in z within a column, so
//             the row a column reports is its first kept row inside the z range: row j writes iff row j - 1 is in another column or below z0.
//   value     one unsigned 64-bit word per cell: d2 << 32 | row, all ones = none.  The lexicographic minimum of (d2, row) is one unsigned min.
//   pass      along one axis: out[i] = min over j in [i - R, i + R] cut to the axis of in[j] + ((i - j)^2 << 32), skipping none.  Three of them, along
//             z (not when planar), y, x, NOT cut at R^2 in between; the last applies the cut d2 <= R^2 and unpacks: dist2, nearest, or -1, -1.
//             The largest value a pass can form is 3 * 128^2 << 32: no carry out of either half.
// Why the three windowed passes give the exact (min d2, lowest row) wherever d2 <= R^2:
//   A site within Euclidean R is within R on every axis.
//   The distance on the other axes is constant along a line.
//   A minimum of minima is the minimum.
// A cell whose nearest site is farther than R may hold any value above the cut between the passes, and none after the last.
#pragma once
#include "accum_columns.h"

#define ACCF_MAX_RADIUS 128
#define ACCF_MAX_CELLS ((int64_t)1 << 28)
#define ACCF_MAX_ORIGIN ((int64_t)1 << 31)            // |x0|, |y0|, |z0| <= this: x0 + i never leaves int64
#define ACCF_NONE 0xffffffffffffffffull

#define ACCF_COUNTERS 4                               // kept rows, sites, cells with a result, cells without one
#define ACCF_C_ROWS 0
#define ACCF_C_SITES 1
#define ACCF_C_NEAR 2
#define ACCF_C_FAR 3

#define ACCF_VALID 1                                  // the status bits of a looked-up row
#define ACCF_INSIDE 2
#define ACCF_NEAR 4
#define ACCF_LOOKUP_COUNTERS 4                        // rows, valid, inside, near

struct AccfBox {
    int64_t x0, y0, z0, nx, ny, nz;
    int planar;
};

PCACC_HD int64_t accf_nz_out(const AccfBox &b) { return b.planar ? 1 : b.nz; }

// The number of cells of a box in range, or -1.  No product is formed before its factors are known to be small.
PCACC_HD int64_t accf_cells(const AccfBox &b)
{
    if (b.x0 < -ACCF_MAX_ORIGIN || b.x0 > ACCF_MAX_ORIGIN || b.y0 < -ACCF_MAX_ORIGIN || b.y0 > ACCF_MAX_ORIGIN || b.z0 < -ACCF_MAX_ORIGIN ||
        b.z0 > ACCF_MAX_ORIGIN)
        return -1;
    if (b.nx < 1 || b.ny < 1 || b.nz < 1 || b.nx > ACCF_MAX_CELLS || b.ny > ACCF_MAX_CELLS || b.nz > ACCF_MAX_ORIGIN) return -1;
    const int64_t plane = b.nx * b.ny;                                                           // <= 2^56
    if (plane > ACCF_MAX_CELLS) return -1;
    const int64_t cells = plane * accf_nz_out(b);                                                // <= 2^59
    return cells > ACCF_MAX_CELLS ? -1 : cells;
}

// Element (i, j, k) of the grid of a box in range; x is slowest, as in the key.
PCACC_HD int64_t accf_cell(const AccfBox &b, int64_t i, int64_t j, int64_t k)
{
    PCACC_BOUND(i, b.nx);
    PCACC_BOUND(j, b.ny);
    PCACC_BOUND(k, accf_nz_out(b));
    return (i * b.ny + j) * accf_nz_out(b) + k;
}

// The cell of voxel c, or -1 when it lies outside the box; planar: z must lie in [z0, z0 + nz) and the cell is that of the column.
PCACC_HD int64_t accf_voxel_cell(const AccfBox &b, const int32_t c[3])
{
    const int64_t i = (int64_t)c[0] - b.x0, j = (int64_t)c[1] - b.y0, k = (int64_t)c[2] - b.z0;
    if (i < 0 || i >= b.nx || j < 0 || j >= b.ny || k < 0 || k >= b.nz) return -1;
    return accf_cell(b, i, j, b.planar ? 0 : k);
}

// The cell that row j of extract() writes its number to, or -1: one writer per cell.
PCACC_HD int64_t accf_site(const AcccMap &M, const AccfBox &b, int64_t j)
{
    const int64_t i = accc_map_row(M, j);
    if (i < 0) return -1;
    int32_t c[3];
    accum_unkey(M.keys[i], c);
    const int64_t cell = accf_voxel_cell(b, c);
    if (cell < 0 || !b.planar || j == 0) return cell;
    const int64_t p = accc_map_row(M, j - 1);
    if (p < 0 || accc_column_key(M.keys[p]) != accc_column_key(M.keys[i])) return cell;
    accum_unkey(M.keys[p], c);
    return (int64_t)c[2] < b.z0 ? cell : -1;                                                     // the row before is the column's first in the range
}

PCACC_HD unsigned long long accf_pack(int64_t d2, int64_t row) { return ((unsigned long long)d2 << 32) | (unsigned long long)(uint32_t)row; }

// What the value v, `delta` steps away along the axis of a pass, offers a cell.
PCACC_HD unsigned long long accf_candidate(unsigned long long v, int64_t delta)
{
    return v == ACCF_NONE ? ACCF_NONE : v + ((unsigned long long)(delta * delta) << 32);
}

// One output of a pass: position i of a line of `len` cells.  Element j of the line stands at line[(j - first) * stride] for j in [first,
// first + count): the whole line in global memory (first = 0, count = len) or the part of it that a chunk holds.  The window is cut to the axis before
// an address is formed; at most 2R + 1 steps.
PCACC_HD unsigned long long accf_line_min(const unsigned long long *line, int64_t stride, int64_t first, int64_t count, int64_t len, int64_t i, int R)
{
    const int64_t lo = i - R < 0 ? 0 : i - R, hi = i + R > len - 1 ? len - 1 : i + R;
    unsigned long long best = ACCF_NONE;
    for (int64_t j = lo; j <= hi; ++j) {
        PCACC_BOUND(j - first, count);
        const unsigned long long v = accf_candidate(line[(j - first) * stride], i - j);
        best = v < best ? v : best;
    }
    return best;
}

// What a workgroup stages of its input before it slides over it (accum_field.hip): `count` elements from `first` on.
struct AccfSpan { int64_t first, count; };

#define ACCF_CHUNK 256                                // contiguous axis: the cells of a chunk, staged with R cells on either side

// Contiguous axis: the cells staged for the chunk [e0, e0 + ACCF_CHUNK) of the flat grid, cut to the grid: at most ACCF_CHUNK + 2R.
PCACC_HD AccfSpan accf_chunk_span(int64_t e0, int R, int64_t cells)
{
    const int64_t s0 = e0 - R < 0 ? 0 : e0 - R, s1 = e0 + ACCF_CHUNK + R > cells ? cells : e0 + ACCF_CHUNK + R;
    const AccfSpan s = {s0, s1 - s0};
    return s;
}

// One output of a pass straight from the grid: cell e of `cells`, the axis has `len` cells `stride` elements apart.
PCACC_HD unsigned long long accf_pass_cell(const unsigned long long *in, int64_t cells, int64_t stride, int64_t len, int64_t e, int R)
{
    PCACC_BOUND(e, cells);
    const int64_t i = (e / stride) % len, base = e - i * stride;
    PCACC_BOUND(base + (len - 1) * stride, cells);
    return accf_line_min(in + base, stride, 0, len, len, i, R);
}

// The cut of the last pass: true and (d2, row) when the value lies within R, else false and (-1, -1).
PCACC_HD bool accf_cut(unsigned long long v, int R, int32_t *d2, int32_t *row)
{
    const bool near = v != ACCF_NONE && (int64_t)(v >> 32) <= (int64_t)R * R;
    *d2 = near ? (int32_t)(v >> 32) : -1;
    *row = near ? (int32_t)(uint32_t)(v & 0xffffffffull) : -1;
    return near;
}

// A row of the lookup: its voxel (valid: C4's rule for a point, the grid for a voxel row) against the two grids of a field call.
PCACC_HD int accf_lookup(bool valid, const int32_t c[3], const AccfBox &b, int64_t cells, const int32_t *dist2, const int32_t *nearest, int32_t *d2, int32_t *row)
{
    *d2 = *row = -1;
    if (!valid) return 0;
    const int64_t cell = accf_voxel_cell(b, c);
    if (cell < 0) return ACCF_VALID;
    PCACC_BOUND(cell, cells);
    if (cell >= cells || dist2[cell] < 0) return ACCF_VALID | ACCF_INSIDE;
    *d2 = dist2[cell];
    *row = nearest[cell];
    return ACCF_VALID | ACCF_INSIDE | ACCF_NEAR;
}

// The voxel of a voxel row: valid iff every index lies in the grid.
PCACC_HD bool accf_coord_valid(const int32_t c[3]) { return accn_in_range(c[0]) && accn_in_range(c[1]) && accn_in_range(c[2]); }
