// C16. The k nearest kept centroids of the accumulated scene cloud within a few voxels (accum_knn.hip; include/pcacc.h C16): of
// a scan point under a pose, or of a kept map row itself (self mode: the base of a statistical outlier removal), as __host__ __device__ functions, so
// that the SAME code runs in the kernels and in a g++ build (tests/accum_knn_host_driver.cpp) where every table index is assert-checked before anything
// runs on a GPU.  Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in the order written here.
// Nothing of C4 - C9 is restated: accr_world, accr_candidate, accn_column, accn_centroid, accn_index, accum_unkey, accum_field are called.
//
// Parameters: radius r in [1, ACCK_MAX_RADIUS] voxels, k in [1, ACCK_MAX_K], max_distance in (0, r * voxel_size]; max_d2 = max_distance * max_distance.
//   query       scan mode: accr_world(T, p, voxel_size, w, idx); false: INVALID, found = 0, padding everywhere.  Never clamped, no key, no address.
//               self mode: kept map row i: w = its float64 centroid (accn_centroid), idx = the voxel of its KEY (accum_unkey, not a floor of the
//               centroid, which may lie 2^-17 m outside the voxel); row i itself is no candidate.
//   candidates  the rows with dst[p] >= 0 (accr_candidate with a NULL flag table: every row the filter keeps) in the (2r+1)^3 voxels around idx: dx = -r..r,
//               inside it dy = -r..r, inside it accn_column's z run with radius r.  Columns outside the grid contribute nothing.  The first column of
//               an x inside the grid is found by accn_column itself, each further one by acck_next_column, which returns accn_column's rows from a
//               search that starts at the end of the last run: the set of candidates is the same, and the result does not depend on their order.
//   distance    d2 = (e_x e_x + e_y e_y) + e_z e_z, e = w - c, c the float64 centroid: accr_match's arithmetic.  Accepted iff d2 <= max_d2.
//   result      the up-to-k accepted candidates with the smallest (d2, row), row = dst[p] = extract's row.  Kept rows ascend with the key, so this IS the
//               order (d2, key): total, hence independent of the order the voxels are visited in; ties go to the lower key.  Written in that ascending
//               order: rows[k] and distance[k] = sqrt(d2), padded with -1 / +inf; found in [0, k]; status = INVALID, or FOUND (found >= 1) | FULL
//               (found == k).  Self mode: mean_distance = (((d_0 + d_1) + d_2) + ...) / found in that order, +inf when found == 0.
// Tables that do not fit (m > capacity) address nothing: every query gets padding.
//
// The running top-k is AcckTop<K>, K = k rounded up to 1, 2, 4, 8 or 16: K named slots that only fully unrolled loops index, so that the kernel keeps
// them in registers (a runtime-indexed array would go to scratch).  acck_insert is one compare-swap chain over the K slots behind one early reject
// against the last slot; only the first k slots are stored.
//
// How far the block reaches.  A centroid is the mean of fixed-point values that each lie within 2^-17 m of a point inside the voxel, so it lies within
// 2^-17 m of the voxel itself.
//   scan mode   the point lies inside voxel idx, the centre of the (2r+1)^3 block: a voxel outside the block is at least r voxel_size away from it, a
//               centroid outside the block farther than r voxel_size - 2^-17.
//   self mode   the query is itself a centroid and may lie 2^-17 m outside its own voxel: a centroid outside the block is farther than
//               r voxel_size - 2^-16.
// For max_distance <= (r - 0.1) voxel_size and voxel sizes of 1 mm and up (0.1 voxel_size >= 1e-4 > 2^-16) no such centroid can be accepted, so the
// result IS the k nearest kept centroids of the whole map within max_distance.  At max_distance = r voxel_size the block search itself is the contract.
#pragma once
#include "accum_register.h"

// The loops over the slots of an AcckTop are fully unrolled in the kernels: every slot index is a compile-time constant.
#if defined(__clang__)
#define ACCK_UNROLL _Pragma("unroll")
#else
#define ACCK_UNROLL
#endif

#define ACCK_MAX_K 16
#define ACCK_MAX_RADIUS 4

#define ACCK_INVALID 1
#define ACCK_FOUND 2
#define ACCK_FULL 4

#define ACCK_COUNTERS 5               // queries, invalid, with at least one neighbour, with k neighbours, neighbours in total
#define ACCK_C_QUERIES 0
#define ACCK_C_INVALID 1
#define ACCK_C_FOUND 2
#define ACCK_C_FULL 3
#define ACCK_C_NEIGHBORS 4

struct AcckParams {                   // named scalars: nothing here is indexed at run time
    const unsigned long long *keys;   // [capacity]           | the first m rows of a map
    const int64_t *acc;               // [ACC_FIELDS][capacity]
    const int *dst;                   // [m]: extract's row of every map row, -1 = filtered out
    int64_t capacity, m;
    double voxel_size, max_d2;
    int radius, k;
};

struct AcckOut {                      // rows and distance are [n][k], the others [n]; mean_distance is NULL in scan mode
    int32_t *rows;
    double *distance;
    int32_t *found;
    uint8_t *status;
    double *mean_distance;
};

template <int K> struct AcckTop {     // ascending in (d2, row); an empty slot is (+inf, -1): every accepted candidate has a finite d2 and sorts before it
    double d2[K];
    int32_t row[K];
};

// k rounded up to the K an AcckTop is instantiated for; 0 for a k outside [1, ACCK_MAX_K].
PCACC_HD int acck_slots(int k)
{
    if (k < 1 || k > ACCK_MAX_K) return 0;
    return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)));
}

template <int K> PCACC_HD void acck_clear(AcckTop<K> &top)
{
    ACCK_UNROLL
    for (int s = 0; s < K; ++s) { top.d2[s] = __builtin_inf(); top.row[s] = -1; }
}

// One accepted candidate (a finite d2, row >= 0).
template <int K> PCACC_HD void acck_insert(AcckTop<K> &top, double d2, int32_t row)
{
    if (!(d2 < top.d2[K - 1] || (d2 == top.d2[K - 1] && row < top.row[K - 1]))) return;        // not among the K smallest so far
    ACCK_UNROLL
    for (int s = 0; s < K; ++s) {                                                                // what a slot gives up moves down the chain
        const bool less = d2 < top.d2[s] || (d2 == top.d2[s] && row < top.row[s]);
        const double td = top.d2[s];
        const int32_t tr = top.row[s];
        top.d2[s] = less ? d2 : td;
        top.row[s] = less ? row : tr;
        d2 = less ? td : d2;
        row = less ? tr : row;
    }
}

// First position in keys[0..m) whose key is >= key, for a `from` in [0, m] below which every key is < key: accum_lower_bound's answer, found by doubling
// steps from `from` and a binary search of the last step.  The columns of one x ascend in the key list and the next one starts a few rows behind the
// last, so this takes a handful of probes next to each other where a search of the whole list takes log2 m far apart.
PCACC_HD int64_t acck_search_from(const unsigned long long *keys, int64_t m, int64_t from, unsigned long long key)
{
    int64_t lo = from < 0 ? 0 : (from > m ? m : from), step = 1;
    while (lo + step <= m) {
        const int64_t q = lo + step - 1;                                                         // in [lo, m)
        PCACC_BOUND(q, m);
        if (!(keys[q] < key)) break;                                                             // the answer lies in [lo, q]
        lo = q + 1;
        step <<= 1;
    }
    const int64_t hi = lo + step - 1 < m ? lo + step - 1 : m;                                    // the answer lies in [lo, hi]
    return lo + accum_lower_bound(keys + lo, hi - lo, key);
}

// accn_column for a column (cx, cy) INSIDE the grid whose keys all lie at or behind position `from` (the end of the run of a column with the same x and
// a lower y): the same run, rows [*first, *first + n), with the search started at `from`.
PCACC_HD int acck_next_column(const unsigned long long *keys, int64_t m, int64_t from, int64_t cx, int64_t cy, int64_t cz, int r, int64_t *first)
{
    const int64_t z_lo = cz - r < -(int64_t)ACC_IDX_BIAS ? -(int64_t)ACC_IDX_BIAS : cz - r;
    const int64_t z_hi = cz + r > (int64_t)ACC_IDX_BIAS - 1 ? (int64_t)ACC_IDX_BIAS - 1 : cz + r;
    const unsigned long long k_hi = accum_key(cx, cy, z_hi);
    const int64_t p0 = acck_search_from(keys, m, from, accum_key(cx, cy, z_lo));
    int n = 0;
    while (n < 2 * r + 1 && p0 + n < m) {
        const int64_t p = accn_index(p0 + n, m);
        if (p < 0 || keys[p] > k_hi) break;
        ++n;
    }
    *first = p0;
    return n;
}

// The accepted candidates of world point w in voxel idx into top; self = the map row that is the query itself, or -1.
template <int K> PCACC_HD void acck_search(const AcckParams &P, const double w[3], const int64_t idx[3], int64_t self, AcckTop<K> &top)
{
    PCACC_NO_CONTRACT
    if (P.m > P.capacity) return;                                                                // tables that do not fit address nothing
    const int r = P.radius;
    for (int dx = -r; dx <= r; ++dx) {
        if (!accn_in_range(idx[0] + dx)) continue;
        int64_t from = -1;                                                                       // the end of the last run of this x; -1: none yet
        for (int dy = -r; dy <= r; ++dy) {
            if (!accn_in_range(idx[1] + dy)) continue;
            int64_t p0;
            const int n = from < 0 ? accn_column(P.keys, P.m, idx[0] + dx, idx[1] + dy, idx[2], r, &p0)
                                   : acck_next_column(P.keys, P.m, from, idx[0] + dx, idx[1] + dy, idx[2], r, &p0);
            from = p0 + n;
            for (int e = 0; e < n; ++e) {
                const int64_t p = accn_index(p0 + e, P.m);
                if (p < 0 || p == self) continue;
                const int64_t j = accr_candidate(P.dst, (const uint8_t *)0, 0, p);
                if (j < 0) continue;
                const int64_t cnt = P.acc[accum_field(0, p, P.capacity)];
                const double cx = accn_centroid(P.acc[accum_field(2, p, P.capacity)], cnt), cy = accn_centroid(P.acc[accum_field(3, p, P.capacity)], cnt),
                             cz = accn_centroid(P.acc[accum_field(4, p, P.capacity)], cnt);
                const double ex = w[0] - cx, ey = w[1] - cy, ez = w[2] - cz;
                const double d2 = (ex * ex + ey * ey) + ez * ez;
                if (!(d2 <= P.max_d2)) continue;
                acck_insert(top, d2, (int32_t)j);
            }
        }
    }
}

// Scan mode: the neighbours of point p under the pose T (rows 0-2 of a row-major 4x4).  -> ACCK_INVALID or 0; top is cleared first.
template <int K> PCACC_HD int acck_point(const AcckParams &P, const double *T, const float *p, AcckTop<K> &top)
{
    acck_clear(top);
    double w[3];
    int64_t idx[3];
    if (!accr_world(T, p, P.voxel_size, w, idx)) return ACCK_INVALID;
    acck_search(P, w, idx, -1, top);
    return 0;
}

// Self mode: the neighbours of map row i (a kept row: dst[i] >= 0).  false (top cleared, nothing addressed) when i is no row of the map.
template <int K> PCACC_HD bool acck_row(const AcckParams &P, int64_t i, AcckTop<K> &top)
{
    acck_clear(top);
    if (accn_index(i, P.m) < 0 || P.m > P.capacity) return false;
    int32_t c[3];
    accum_unkey(P.keys[i], c);
    const int64_t cnt = P.acc[accum_field(0, i, P.capacity)];
    const double w[3] = {accn_centroid(P.acc[accum_field(2, i, P.capacity)], cnt), accn_centroid(P.acc[accum_field(3, i, P.capacity)], cnt),
                         accn_centroid(P.acc[accum_field(4, i, P.capacity)], cnt)};
    const int64_t idx[3] = {c[0], c[1], c[2]};
    acck_search(P, w, idx, i, top);
    return true;
}

// Row i of every output column, each written once: the first k slots of top.  -> found, or -1 (nothing addressed) when i is no row.
template <int K> PCACC_HD int acck_store(const AcckOut &o, int64_t i, int64_t n, int k, const AcckTop<K> &top, int status)
{
    PCACC_NO_CONTRACT
    if (accn_index(i, n) < 0 || k < 1 || k > K) return -1;
    int found = 0;
    double sum = 0.0;
    ACCK_UNROLL
    for (int s = 0; s < K; ++s) {
        if (s >= k) continue;
        const bool have = !(status & ACCK_INVALID) && top.row[s] >= 0;
        const double d = have ? __builtin_sqrt(top.d2[s]) : __builtin_inf();
        o.rows[i * k + s] = have ? top.row[s] : -1;
        o.distance[i * k + s] = d;
        if (have) {
            sum = found ? sum + d : d;
            ++found;
        }
    }
    if (found > 0) status |= ACCK_FOUND;
    if (found == k) status |= ACCK_FULL;
    o.found[i] = found;
    o.status[i] = (uint8_t)status;
    if (o.mean_distance) o.mean_distance[i] = found ? sum / (double)found : __builtin_inf();
    return found;
}
