// C11. Connected components of the accumulated scene cloud (accum_components.hip; include/pcacc.h C11): which rows take part, the
// edges of one row, the contribution of one row to its component, how two contributions combine and which rows a removal drops, as __host__ __device__
// functions, so that the SAME code runs in the kernels and in a g++ build (tests/accum_components_host_driver.cpp) where every table index is
// assert-checked before anything runs on a GPU.  Includes nothing of HIP; calls the helpers of sections 9c-9g (accum_unkey, accum_field, accn_index,
// accn_column, accn_centroid, accum_merge_dst, accr_move_row) and restates none.  The only floating-point operation is accn_centroid's.
//
//   rows        map row i takes part iff dst[i] >= 0 (the row table of accn_rows_launch under (min_count, max_moving_fraction): extract's row j of
//               map row i) and, with a mask, mask[dst[i]] != 0.  mask_rows != kept: nothing takes part (BAD_MASK), decided on the device.
//   edges       two rows that take part are adjacent iff |delta|_inf <= radius.  Row i visits the columns (dx, dy) whose keys can lie below its own
//               (dx < 0, or dx = 0 and dy <= 0) with accn_column and reports every row p < i that takes part: each edge once, from its larger end.
//               An offset that leaves [-2^20, 2^20) is skipped before a key is formed (accn_column).
//   labels      the union-find of union_find.h on EXTRACT rows: the root of a set is its smallest extract row = its smallest key.  Components are
//               numbered 0 .. K-1 in ascending order of that row: the exclusive scan of the root flags.
//   statistics  integers only: sums (64 bit), minima and maxima (32 bit) -- they commute, so a table does not depend on the order of its terms.
//               sum_q cannot overflow: |q| < 2^31 per point (ACC_COORD_LIMIT) and a map holds fewer than 2^31 points (the bound of a record's
//               count), so |sum q_a| < 2^62.
//   removal     a row that takes part is SMALL iff its component has voxels < min_voxels or points < min_points (a threshold of 0 is off).  Rows that
//               do not take part stay.  Survivor i moves, record unchanged, to row accum_merge_dst(survivors below it, 0, kept) of the other tables.
#pragma once
#include "accum_prune.h"
#include "union_find.h"

#define ACCC_COUNTERS 7
#define ACCC_C_ROWS 0
#define ACCC_C_PARTICIPATING 1
#define ACCC_C_OUTSIDE 2
#define ACCC_C_MASKED 3
#define ACCC_C_COMPONENTS 4
#define ACCC_C_LARGEST 5
#define ACCC_C_STATUS 6
#define ACCC_OK 0
#define ACCC_BAD_MASK 1
#define ACCC_GAVE_UP 2
#define ACCC_REMOVE_COUNTERS 4
#define ACCC_R_KEPT 0
#define ACCC_R_SMALL 1
#define ACCC_R_COMPONENTS_REMOVED 2
#define ACCC_R_COMPONENTS_KEPT 3
#define ACCC_OUTSIDE (-1)                // accc_row: the filter does not keep the row
#define ACCC_MASKED (-2)                 // accc_row: the mask excludes the row
#define ACCC_UNION_TRIES 1024            // attempts of one join's CAS before the kernel gives up (status GAVE_UP)
#define ACCC_I32_MAX 0x7fffffff
#define ACCC_I32_MIN (-0x7fffffff - 1)

// mask == NULL or a mask of exactly `kept` rows.
PCACC_HD bool accc_mask_fits(const uint8_t *mask, int64_t mask_rows, int64_t kept) { return mask == nullptr || mask_rows == kept; }

// Extract row j in [0, kept) takes part (the mask has been found to fit).
PCACC_HD bool accc_takes_part(const uint8_t *mask, int64_t kept, int64_t j)
{
    if (accn_index(j, kept) < 0) return false;
    return mask == nullptr || mask[j] != 0;
}

// Map row i: its extract row when it takes part, else ACCC_OUTSIDE / ACCC_MASKED.  No row of the map: ACCC_OUTSIDE, nothing addressed.
PCACC_HD int64_t accc_row(const int *dst, const uint8_t *mask, int64_t kept, int64_t i, int64_t m)
{
    if (i < 0 || i >= m) return ACCC_OUTSIDE;
    const int64_t j = dst[accn_index(i, m)];
    if (j < 0 || j >= kept) return ACCC_OUTSIDE;
    return accc_takes_part(mask, kept, j) ? j : ACCC_MASKED;
}

// The edges of map row i (which takes part, extract row j): visit(j, extract row of p) for every row p < i that takes part and lies within
// `radius` voxels.  -> the number of edges reported.
template <class Visit>
PCACC_HD int accc_edges(const unsigned long long *keys, int64_t m, const int *dst, const uint8_t *mask, int64_t kept, int64_t i, int64_t j, int radius,
                        Visit &&visit)
{
    if (accn_index(i, m) < 0) return 0;
    int32_t c[3];
    accum_unkey(keys[i], c);
    int n_edges = 0;
    for (int dx = -radius; dx <= 0; ++dx)
        for (int dy = -radius; dy <= (dx < 0 ? radius : 0); ++dy) {            // every other column holds larger keys only
            int64_t p0;
            const int n = accn_column(keys, m, (int64_t)c[0] + dx, (int64_t)c[1] + dy, c[2], radius, &p0);
            for (int e = 0; e < n; ++e) {
                const int64_t p = accn_index(p0 + e, m);
                if (p < 0 || p >= i) continue;
                const int64_t q = accc_row(dst, mask, kept, p, m);
                if (q < 0) continue;
                visit(j, q);
                ++n_edges;
            }
        }
    return n_edges;
}

// What one row, or a set of rows of one component, adds to the component's record.  Named scalars: nothing here is indexed at run time.
struct AcccStat {
    int64_t voxels, points, moving, sq_x, sq_y, sq_z;
    int32_t lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, t_first, t_last;
};

PCACC_HD void accc_stat_none(AcccStat *s)
{
    s->voxels = s->points = s->moving = s->sq_x = s->sq_y = s->sq_z = 0;
    s->lo_x = s->lo_y = s->lo_z = s->t_first = ACCC_I32_MAX;
    s->hi_x = s->hi_y = s->hi_z = s->t_last = ACCC_I32_MIN;
}

// The contribution of map row i; false (and *s = none, nothing addressed) when i is no row of the map.
PCACC_HD bool accc_stat_row(const unsigned long long *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t i, AcccStat *s)
{
    accc_stat_none(s);
    if (i < 0 || i >= m || m > capacity) return false;
    PCACC_BOUND(i, capacity);
    int32_t c[3];
    accum_unkey(keys[i], c);
    s->voxels = 1;
    s->points = acc[accum_field(0, i, capacity)];
    s->moving = acc[accum_field(1, i, capacity)];
    s->sq_x = acc[accum_field(2, i, capacity)];
    s->sq_y = acc[accum_field(3, i, capacity)];
    s->sq_z = acc[accum_field(4, i, capacity)];
    s->lo_x = s->hi_x = c[0];
    s->lo_y = s->hi_y = c[1];
    s->lo_z = s->hi_z = c[2];
    s->t_first = stamps[i];
    s->t_last = stamps[capacity + i];
    return true;
}

PCACC_HD int32_t accc_min(int32_t a, int32_t b) { return b < a ? b : a; }
PCACC_HD int32_t accc_max(int32_t a, int32_t b) { return b > a ? b : a; }

// a <- a and b together: every field commutes and associates.
PCACC_HD void accc_stat_merge(AcccStat *a, const AcccStat &b)
{
    a->voxels += b.voxels; a->points += b.points; a->moving += b.moving; a->sq_x += b.sq_x; a->sq_y += b.sq_y; a->sq_z += b.sq_z;
    a->lo_x = accc_min(a->lo_x, b.lo_x); a->lo_y = accc_min(a->lo_y, b.lo_y); a->lo_z = accc_min(a->lo_z, b.lo_z);
    a->hi_x = accc_max(a->hi_x, b.hi_x); a->hi_y = accc_max(a->hi_y, b.hi_y); a->hi_z = accc_max(a->hi_z, b.hi_z);
    a->t_first = accc_min(a->t_first, b.t_first); a->t_last = accc_max(a->t_last, b.t_last);
}

// The float32 centroid of a component on one axis (points > 0: a component has a voxel, a kept voxel a point).
PCACC_HD float accc_centroid(int64_t sum_q, int64_t points) { return (float)accn_centroid(sum_q, points); }

PCACC_HD bool accc_small(int64_t voxels, int64_t points, int64_t min_voxels, int64_t min_points)
{
    return (min_voxels > 0 && voxels < min_voxels) || (min_points > 0 && points < min_points);
}

// Map row i leaves the map: it takes part (label[dst[i]] >= 0) and its component is small.  label [kept], voxels / points [n_components];
// a label that names no component removes nothing.
PCACC_HD bool accc_row_small(const int *dst, const int32_t *label, const int32_t *voxels, const int64_t *points, int64_t kept, int64_t n_components,
                             int64_t i, int64_t m, int64_t min_voxels, int64_t min_points)
{
    if (i < 0 || i >= m) return false;
    const int64_t j = dst[accn_index(i, m)];
    if (j < 0 || j >= kept) return false;
    const int64_t c = label[accn_index(j, kept)];
    if (c < 0 || c >= n_components) return false;
    PCACC_BOUND(c, n_components);
    return accc_small(voxels[c], points[c], min_voxels, min_points);
}
