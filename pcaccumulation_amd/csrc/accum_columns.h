// C17. The (x, y) columns of the accumulated scene cloud: what stands on the ground, how high above it, and bird's-eye-view rasters (accum_columns.hip;
// include/pcacc.h C17), as __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build
// (tests/accum_columns_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.  Includes nothing of HIP.
// Nothing of C4 - C5 is restated: accum_unkey, accum_lower_bound, accum_field, accum_centroid, accn_index, accn_in_range, accn_centroid are called.
//
// Keys ascend lexicographically in (x, y, z), so the kept voxels of one (x, y) are a run of consecutive rows of extract(), ascending in z: no sort and
// no hash table.  Everything below is over the rows extract's filter keeps (rows[kept] of pass 1 of C5); j denotes a row of extract().
//   column key    key >> 21: (x + 2^20) << 21 | (y + 2^20), 42 bits, ascending = lexicographic (x, y)
//   head          row j is a head iff j == 0 or its column key differs from that of row j - 1; columns are numbered in key order, C of them
//   per column c  xy; first_row (the head) and voxels: the column is rows [first_row, first_row + voxels); points = sum count, moving = sum moving;
//                 z_low, z_high = the voxel index z of the first and the last row of the run; t_first = min, t_last = max of the stamps
//   ground        ground_z(c) = min z_low(c') over the columns c' that exist with |dx| <= R and |dy| <= R, R in [0, ACCC_MAX_RADIUS], c itself
//                 included.  The supplier minimises the pair (z_low, column key): a total order, ties go to the lower key.  ground_row(c) = the
//                 supplier's first_row, ground_column(c) = its index.  A neighbour column outside [-2^20, 2^20) contributes nothing and forms NO key:
//                 x + dx is tested before anything else, y - R and y + R are cut to the grid, so no field of a key can wrap into the next.
//                 Per dx one accum_lower_bound on (x + dx, y_lo) in the column-key list and a walk over at most 2R + 1 consecutive columns while
//                 x is still x + dx and y <= y_hi (the y field of the next x follows directly in the list).
//   band          0 <= band_lo <= band_hi < 2^21: band_voxels(c) = rows of the column with band_lo <= z - ground_z(c) <= band_hi, band_top(c) the
//                 largest such z - ground_z(c), or -1
//   per row j     column; height = z - ground_z(column) >= 0 (the own column is a candidate and z >= its z_low); is_ground = height <= thickness,
//                 thickness in [0, 2^21); height_m = accn_centroid(sum q_z, count) of row j MINUS the same of ground_row(column): one float64
//                 subtraction.  It may be slightly negative: a centroid can lie 2^-17 m outside its voxel, so two voxels at equal z, or a row
//                 and a ground row one voxel apart, can come out up to 2^-16 m the other way round.
//   pixel         (r, c) of a W x H window at the integer origin (x0, y0) is column (x0 + c, y0 + r).  A column outside the grid forms no key; one
//                 that is not in the list is empty: column -1, elevation and ground NaN, band_top -1, voxels 0.  Otherwise elevation =
//                 accum_centroid z of row first_row + voxels - 1, ground = accum_centroid z of ground_row (extract's float32 bits).
// All results are integers except height_m and the two float32 of a pixel, each one fixed sequence of IEEE operations with no FMA contraction.
#pragma once
#include "accum_normals.h"

#define ACCC_MAX_RADIUS 8
#define ACCC_MAX_HEIGHT 2097151                       // 2^21 - 1: thickness and the band bounds
#define ACCC_MAX_PIXELS ((int64_t)1 << 28)
#define ACCC_MAX_ORIGIN ((int64_t)1 << 31)            // |x0|, |y0| <= this: x0 + c never leaves int64

#define ACCC_COUNTERS 5                               // kept rows, columns, ground rows, rows in the band, columns whose ground came from another column
#define ACCC_C_ROWS 0
#define ACCC_C_COLUMNS 1
#define ACCC_C_GROUND 2
#define ACCC_C_BAND 3
#define ACCC_C_BORROWED 4

struct AcccMap {                                      // the first m rows of a map and the rows the filter keeps
    const unsigned long long *keys;                   // [capacity]
    const int64_t *acc;                               // [ACC_FIELDS][capacity]
    const int32_t *stamps;                            // [2][capacity]; NULL where no stamp is read (the pixels)
    const int *rows;                                  // [kept]: the map row of every row of extract()
    int64_t capacity, m, kept;
};

struct AcccColumn {                                   // what the column kernel writes of one column
    unsigned long long key;
    int32_t xy[2];
    int32_t first_row, voxels;
    int64_t points, moving;
    int32_t z_low, z_high, t_first, t_last;
};

struct AcccColumns {                                  // the column tables a pixel reads, C rows each
    const unsigned long long *key;
    const int32_t *first_row, *voxels, *ground_row, *band_top;
    int64_t C;
};

struct AcccPixel {
    int32_t column;
    float elevation, ground;
    int32_t band_top, voxels;
};

PCACC_HD unsigned long long accc_column_key(unsigned long long key) { return key >> 21; }

// The column key of (x, y), both inside the grid.
PCACC_HD unsigned long long accc_xy_key(int64_t x, int64_t y)
{
    return ((unsigned long long)(x + ACC_IDX_BIAS) << 21) | (unsigned long long)(y + ACC_IDX_BIAS);
}

// The map row of row j of extract(), or -1 (nothing is addressed) when j is no kept row or the tables do not fit.
PCACC_HD int64_t accc_map_row(const AcccMap &M, int64_t j)
{
    if (j < 0 || j >= M.kept || M.kept > M.m || M.m > M.capacity) return -1;
    const int64_t i = M.rows[accn_index(j, M.kept)];
    return (i >= 0 && i < M.m) ? accn_index(i, M.m) : -1;
}

PCACC_HD bool accc_is_head(const AcccMap &M, int64_t j)
{
    const int64_t i = accc_map_row(M, j);
    if (i < 0) return false;
    if (j == 0) return true;
    const int64_t p = accc_map_row(M, j - 1);
    return p < 0 || accc_column_key(M.keys[p]) != accc_column_key(M.keys[i]);
}

// The column whose head is row j: one walk over its run.  false (nothing written) when j is no kept row.
PCACC_HD bool accc_column(const AcccMap &M, int64_t j, AcccColumn *out)
{
    const int64_t i0 = accc_map_row(M, j);
    if (i0 < 0) return false;
    int32_t c[3];
    accum_unkey(M.keys[i0], c);
    const unsigned long long ck = accc_column_key(M.keys[i0]);
    out->key = ck;
    out->xy[0] = c[0]; out->xy[1] = c[1];
    out->first_row = (int32_t)j;
    out->z_low = out->z_high = c[2];
    out->points = out->moving = 0;
    out->t_first = M.stamps[i0];
    out->t_last = M.stamps[M.capacity + i0];
    int32_t n = 0;
    for (int64_t e = j; e < M.kept; ++e) {
        const int64_t i = accc_map_row(M, e);
        if (i < 0 || accc_column_key(M.keys[i]) != ck) break;
        PCACC_BOUND(M.capacity + i, 2 * M.capacity);
        accum_unkey(M.keys[i], c);
        out->z_high = c[2];                                                                      // the rows of a run ascend in z
        out->points += M.acc[accum_field(0, i, M.capacity)];
        out->moving += M.acc[accum_field(1, i, M.capacity)];
        const int32_t a = M.stamps[i], b = M.stamps[M.capacity + i];
        out->t_first = a < out->t_first ? a : out->t_first;
        out->t_last = b > out->t_last ? b : out->t_last;
        ++n;
    }
    out->voxels = n;
    return true;
}

// The supplier of the ground of column c: the column that minimises (z_low, column key) among the existing columns within R of c on both axes.
// In [0, C), or -1 (nothing addressed) when c is no column.
PCACC_HD int64_t accc_ground(const unsigned long long *col_key, const int32_t *z_low, int64_t C, int64_t c, int R)
{
    if (c < 0 || c >= C) return -1;
    const int64_t own = accn_index(c, C);
    const int64_t x = (int64_t)(col_key[own] >> 21) - ACC_IDX_BIAS, y = (int64_t)(col_key[own] & 0x1fffff) - ACC_IDX_BIAS;
    int64_t best = own;
    int32_t best_z = z_low[own];
    unsigned long long best_key = col_key[own];
    const int64_t y_lo = y - R < -(int64_t)ACC_IDX_BIAS ? -(int64_t)ACC_IDX_BIAS : y - R;      // cut to the grid BEFORE a key is formed
    const int64_t y_hi = y + R > (int64_t)ACC_IDX_BIAS - 1 ? (int64_t)ACC_IDX_BIAS - 1 : y + R;
    for (int dx = -R; dx <= R; ++dx) {
        const int64_t cx = x + dx;
        if (!accn_in_range(cx)) continue;                                                        // no key: x - R below the grid would borrow from nothing
        const int64_t p0 = accum_lower_bound(col_key, C, accc_xy_key(cx, y_lo));
        for (int n = 0; n < 2 * R + 1 && p0 + n < C; ++n) {
            const int64_t p = accn_index(p0 + n, C);
            const int64_t px = (int64_t)(col_key[p] >> 21) - ACC_IDX_BIAS, py = (int64_t)(col_key[p] & 0x1fffff) - ACC_IDX_BIAS;
            if (px != cx || py > y_hi) break;                                                    // the next x starts at ITS lowest y: never a neighbour
            const int32_t z = z_low[p];
            if (z < best_z || (z == best_z && col_key[p] < best_key)) { best = p; best_z = z; best_key = col_key[p]; }
        }
    }
    return best;
}

// The rows of the column [first_row, first_row + voxels) in the band above ground_z: -> their number, *top = the largest height among them or -1.
PCACC_HD int32_t accc_band(const AcccMap &M, int64_t first_row, int32_t voxels, int32_t ground_z, int32_t band_lo, int32_t band_hi, int32_t *top)
{
    int32_t n = 0;
    *top = -1;
    for (int32_t e = 0; e < voxels; ++e) {
        const int64_t i = accc_map_row(M, first_row + e);
        if (i < 0) break;
        int32_t c[3];
        accum_unkey(M.keys[i], c);
        const int32_t h = c[2] - ground_z;
        if (h >= band_lo && h <= band_hi) { ++n; *top = h; }                                     // ascending in z: the last one is the largest
    }
    return n;
}

// height_m of row j over the row `ground_row` of extract(): one subtraction of two float64 centroids.  NaN when either is no kept row.
PCACC_HD double accc_height_m(const AcccMap &M, int64_t j, int64_t ground_row)
{
    PCACC_NO_CONTRACT
    const int64_t i = accc_map_row(M, j), g = accc_map_row(M, ground_row);
    if (i < 0 || g < 0) return __builtin_nan("");
    const double z = accn_centroid(M.acc[accum_field(4, i, M.capacity)], M.acc[accum_field(0, i, M.capacity)]);
    const double z0 = accn_centroid(M.acc[accum_field(4, g, M.capacity)], M.acc[accum_field(0, g, M.capacity)]);
    return z - z0;
}

// The voxel index z of row j of extract(); false when j is no kept row.
PCACC_HD bool accc_row_z(const AcccMap &M, int64_t j, int32_t *z)
{
    const int64_t i = accc_map_row(M, j);
    if (i < 0) return false;
    int32_t c[3];
    accum_unkey(M.keys[i], c);
    *z = c[2];
    return true;
}

// extract's float32 z of row j of extract(), NaN when j is no kept row.
PCACC_HD float accc_row_z32(const AcccMap &M, int64_t j)
{
    const int64_t i = accc_map_row(M, j);
    if (i < 0) return __builtin_nanf("");
    return accum_centroid(M.acc[accum_field(4, i, M.capacity)], M.acc[accum_field(0, i, M.capacity)]);
}

// The column of (x, y) in the list: its index, or -1.  A column outside the grid forms no key; nothing outside [0, C) is searched.
PCACC_HD int64_t accc_find_column(const unsigned long long *col_key, int64_t C, int64_t x, int64_t y)
{
    if (!accn_in_range(x) || !accn_in_range(y) || C <= 0) return -1;
    const unsigned long long k = accc_xy_key(x, y);
    const int64_t p = accum_lower_bound(col_key, C, k);
    if (p >= C) return -1;
    return col_key[accn_index(p, C)] == k ? p : -1;
}

// The whole pixel of column (x, y).
PCACC_HD void accc_pixel(const AcccMap &M, const AcccColumns &T, int64_t x, int64_t y, AcccPixel *out)
{
    const int64_t c = accc_find_column(T.key, T.C, x, y);
    out->column = (int32_t)c;
    if (c < 0) {
        out->elevation = out->ground = __builtin_nanf("");
        out->band_top = -1;
        out->voxels = 0;
        return;
    }
    PCACC_BOUND(c, T.C);
    out->elevation = accc_row_z32(M, (int64_t)T.first_row[c] + T.voxels[c] - 1);
    out->ground = accc_row_z32(M, T.ground_row[c]);
    out->band_top = T.band_top[c];
    out->voxels = T.voxels[c];
}
