// C8. Removing rows from the accumulated scene cloud (accum_prune.hip; include/pcacc.h C8): the reason a row leaves the map, the
// neighbour count of a survivor and the move of one surviving row as __host__ __device__ functions, so that the SAME code runs in the kernels and in a
// g++ build (tests/accum_prune_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.  The only floating-point operations are the two divisions of accum_keep and of the pierced ratio: both builds give the same integers.
//
// Stage A, per row, from that row's record alone -- the first test that holds is the row's reason:
//   FILTER     !accum_keep(count, moving, min_count, use_fraction, max_moving_fraction)        extract's predicate, called
//   STALE      use_stamp && t_last < before_stamp
//   BOX        use_box && a voxel index of accum_unkey(key) lies outside [lo_a, hi_a]            integer voxel indices, inclusive
//   PIERCED    min_pierced > 0, a sidecar, p = pierced[row] >= min_pierced and, with use_ratio, (double)p / (double)count > ratio (strict)
// Stage B (min_neighbors > 0), per stage-A survivor: k = stage-A survivors with |delta|_inf <= radius, itself included, found as section 9d finds
// neighbours (accn_column per (dx, dy) column, dst[row] >= 0 as the neighbour test; offsets that leave [-2^20, 2^20) are skipped before a key is
// formed).  ISOLATED iff k < min_neighbors.  One pass: k counts stage-A survivors, never stage-B survivors -- a function of the map alone.
// A surviving row moves, record unchanged, to row accum_merge_dst(survivors below it, 0, kept) of the other table set.
#pragma once
#include "accum_normals.h"

#define ACCR_REASONS 6
#define ACCR_KEPT 0
#define ACCR_FILTER 1
#define ACCR_STALE 2
#define ACCR_BOX 3
#define ACCR_PIERCED 4
#define ACCR_ISOLATED 5
#define ACCR_MAX_NEIGHBORS 343          // (2 * 3 + 1)^3: more than this no voxel has

struct AccrParams {                     // named scalars: nothing here is indexed at run time
    int64_t min_count;
    double max_moving_fraction, ratio;
    int32_t before_stamp, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, min_pierced;
    int use_fraction, use_stamp, use_box, use_ratio;
};

// Stage A on the values of one record; has_pierced = a sidecar was given (p is its entry, else ignored).
PCACC_HD int accr_reason(const AccrParams &P, int64_t count, int64_t moving, int32_t t_last, unsigned long long key, bool has_pierced, int32_t p)
{
    if (!accum_keep(count, moving, P.min_count, P.use_fraction != 0, P.max_moving_fraction)) return ACCR_FILTER;
    if (P.use_stamp && t_last < P.before_stamp) return ACCR_STALE;
    if (P.use_box) {
        int32_t c[3];
        accum_unkey(key, c);
        if (c[0] < P.lo_x || c[0] > P.hi_x || c[1] < P.lo_y || c[1] > P.hi_y || c[2] < P.lo_z || c[2] > P.hi_z) return ACCR_BOX;
    }
    if (P.min_pierced > 0 && has_pierced && p >= P.min_pierced) {
        if (!P.use_ratio || (double)p / (double)count > P.ratio) return ACCR_PIERCED;                // count > 0: accum_keep held
    }
    return ACCR_KEPT;
}

// Stage A of map row i; pierced may be NULL.  ACCR_FILTER (nothing addressed) when i is no row of the map.
PCACC_HD int accr_row_reason(const unsigned long long *keys, const int64_t *acc, const int32_t *stamps, const int32_t *pierced, int64_t capacity, int64_t m,
                             int64_t i, const AccrParams &P)
{
    if (accn_index(i, m) < 0 || m > capacity) return ACCR_FILTER;
    PCACC_BOUND(i, capacity);
    return accr_reason(P, acc[accum_field(0, i, capacity)], acc[accum_field(1, i, capacity)], stamps[capacity + i], keys[i], pierced != nullptr,
                       pierced ? pierced[i] : 0);
}

// Stage B of map row i (a stage-A survivor: dst[i] >= 0): the survivors in the (2r+1)^3 voxels around it.  dst[m]: >= 0 for a stage-A survivor.
PCACC_HD int accr_neighbors(const unsigned long long *keys, int64_t m, const int *dst, int64_t i, int radius)
{
    if (accn_index(i, m) < 0) return 0;
    int32_t c[3];
    accum_unkey(keys[i], c);
    int k = 0;
    for (int dx = -radius; dx <= radius; ++dx)
        for (int dy = -radius; dy <= radius; ++dy) {
            int64_t p0;
            const int n = accn_column(keys, m, (int64_t)c[0] + dx, (int64_t)c[1] + dy, c[2], radius, &p0);
            for (int e = 0; e < n; ++e) {
                const int64_t p = accn_index(p0 + e, m);
                if (p >= 0 && dst[p] >= 0) ++k;
            }
        }
    return k;
}

// Row i of the input tables to row d of the output tables, column by column; in_pierced / out_pierced both given or both NULL.
// false (nothing addressed) when i or d is no row.
PCACC_HD bool accr_move_row(const unsigned long long *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                            int64_t m, int64_t i, unsigned long long *out_keys, int64_t *out_acc, int32_t *out_stamps, int32_t *out_pierced,
                            int64_t out_capacity, int64_t kept, int64_t d)
{
    if (i < 0 || i >= m || m > in_capacity || d < 0 || d >= kept || kept > out_capacity) return false;
    PCACC_BOUND(i, in_capacity);
    PCACC_BOUND(d, out_capacity);
    out_keys[d] = in_keys[i];
    for (int f = 0; f < ACC_FIELDS; ++f) out_acc[accum_field(f, d, out_capacity)] = in_acc[accum_field(f, i, in_capacity)];
    out_stamps[d] = in_stamps[i];
    out_stamps[out_capacity + d] = in_stamps[in_capacity + i];
    if (in_pierced && out_pierced) out_pierced[d] = in_pierced[i];
    return true;
}
