// C12. Two accumulated scene clouds into one, and a map under a rigid pose and / or a new voxel size (accum_merge.hip; include/pcacc.h C12, DESIGN.md
// section 9l): the search of one map's row in the other, the move of a row of either map to its row of the union, and the key and the contribution of a
// map row that is re-voxelised, as __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build
// (tests/accum_merge_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.
//
// merge   A (ma rows) and B (mb rows), both ascending and duplicate-free, on ONE grid.  B row j: p = accum_lower_bound(A, key), miss iff A lacks the key;
//         mrank = exclusive scan of the misses.  A row p -> row p + mrank[accum_lower_bound(B, key)] of the union, its record plus B's when B holds the
//         key (integer sums, stamps min / max, ray counts summed in int64 and stored as min(sum, 2^31 - 1)); missed B row j -> row p + mrank[j], copied.
// regrid  a row is `count` points at its float64 centroid (lossy by design).  Usable iff 0 < count <= 2^31; c_a = accn_centroid(sum q_a, count);
//         w_a, validity, voxel index, key and q_a by C4's rules on the float64 centroid (accum_point64: accum_point with a float64 input);
//         contribution count, moving, count * q_a (|.| < 2^62), both stamps, the ray count.  An unusable or invalid row is never clamped and forms no
//         address.
#pragma once
#include "accum_normals.h"

#define ACCM_PIERCED_MAX 2147483647ll               // a stored ray count: int32
#define ACCG_COUNT_MAX ((int64_t)1 << 31)           // count * q stays below 2^62

// accum_point for a float64 point: the same operations and the same checks in the same order.
PCACC_HD bool accum_point64(const double *T, const double *p, double voxel_size, unsigned long long *key, int64_t q[3])
{
    PCACC_NO_CONTRACT
    const double x = p[0], y = p[1], z = p[2];
    int64_t idx[3];
    for (int a = 0; a < 3; ++a) {
        const double w = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
        if (!pcacc_finite(w) || !(__builtin_fabs(w) < ACC_COORD_LIMIT)) return false;
        const double c = __builtin_floor(w / voxel_size);
        if (!(c >= -(double)ACC_IDX_BIAS && c < (double)ACC_IDX_BIAS)) return false;
        idx[a] = (int64_t)c;
        q[a] = (int64_t)__builtin_rint(w * ACC_FIXED_ONE);
    }
    *key = accum_key(idx[0], idx[1], idx[2]);
    return true;
}

// min(sum, 2^31 - 1) of two ray counts (each a stored int32 or a sum of them); *saturated = 1 when the sum did not fit.
PCACC_HD int32_t accm_pierced(int64_t sum, int *saturated)
{
    *saturated = sum > ACCM_PIERCED_MAX ? 1 : 0;
    return (int32_t)(sum > ACCM_PIERCED_MAX ? ACCM_PIERCED_MAX : sum);
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------------------------
// B row j in A's keys: *pos = A keys below it, in [0, ma]; -> 1 when A lacks the key.  Nothing is addressed when j is no row of B.
PCACC_HD int accm_search(const unsigned long long *a_keys, int64_t ma, const unsigned long long *b_keys, int64_t mb, int64_t j, int64_t *pos)
{
    *pos = 0;
    if (j < 0 || j >= mb) return 0;
    PCACC_BOUND(j, mb);
    const unsigned long long key = b_keys[j];
    const int64_t p = accum_lower_bound(a_keys, ma, key);
    *pos = p;
    if (p < ma) { PCACC_BOUND(p, ma); }
    return !(p < ma && a_keys[p] == key);
}

#define ACCM_WRITTEN 1
#define ACCM_SHARED 2
#define ACCM_SATURATED 4

// A row p to its row of the union; mrank has mrank_n >= mb + 1 entries.  a_pierced / b_pierced may be NULL (that side counts 0 rays); out_pierced is
// written when given.  -> a sum of ACCM_* bits, 0 (nothing addressed) when p is no row or the destination does not fit.
PCACC_HD int accm_old_row(const unsigned long long *a_keys, const int64_t *a_acc, const int32_t *a_stamps, const int32_t *a_pierced, int64_t a_capacity,
                          int64_t ma, const unsigned long long *b_keys, const int64_t *b_acc, const int32_t *b_stamps, const int32_t *b_pierced,
                          int64_t b_capacity, int64_t mb, const int *mrank, int64_t mrank_n, int64_t p, unsigned long long *out_keys, int64_t *out_acc,
                          int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t total)
{
    if (p < 0 || p >= ma || ma > a_capacity || mb > b_capacity || mb >= mrank_n || total > out_capacity) return 0;
    PCACC_BOUND(p, a_capacity);
    const unsigned long long key = a_keys[p];
    const int64_t j = accum_lower_bound(b_keys, mb, key);                        // in [0, mb]
    PCACC_BOUND(j, mrank_n);
    const int64_t d = accum_merge_dst(p, mrank[j], total);
    if (d < 0) return 0;
    PCACC_BOUND(d, out_capacity);
    const bool hit = j < mb && b_keys[j] == key;
    int flags = ACCM_WRITTEN | (hit ? ACCM_SHARED : 0);
    out_keys[d] = key;
    for (int f = 0; f < ACC_FIELDS; ++f)
        out_acc[accum_field(f, d, out_capacity)] = a_acc[accum_field(f, p, a_capacity)] + (hit ? b_acc[accum_field(f, j, b_capacity)] : 0);
    const int32_t t0 = a_stamps[p], t1 = a_stamps[a_capacity + p];
    if (hit) {
        PCACC_BOUND(j, b_capacity);
        const int32_t u0 = b_stamps[j], u1 = b_stamps[b_capacity + j];
        out_stamps[d] = u0 < t0 ? u0 : t0;
        out_stamps[out_capacity + d] = u1 > t1 ? u1 : t1;
    } else {
        out_stamps[d] = t0;
        out_stamps[out_capacity + d] = t1;
    }
    if (out_pierced) {
        const int64_t ra = a_pierced ? a_pierced[p] : 0, rb = (hit && b_pierced) ? b_pierced[j] : 0;
        int sat = 0;
        out_pierced[d] = hit ? accm_pierced(ra + rb, &sat) : (int32_t)ra;            // a key of one map only: copied bit for bit
        if (sat) flags |= ACCM_SATURATED;
    }
    return flags;
}

// Missed B row j (A lacks its key, pos A keys below it) to row pos + mrank[j] of the union, copied.  -> ACCM_WRITTEN or 0 (nothing addressed).
PCACC_HD int accm_new_row(const unsigned long long *b_keys, const int64_t *b_acc, const int32_t *b_stamps, const int32_t *b_pierced, int64_t b_capacity,
                          int64_t mb, const int *mrank, int64_t mrank_n, int64_t j, int64_t pos, unsigned long long *out_keys, int64_t *out_acc,
                          int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t total)
{
    if (j < 0 || j >= mb || mb > b_capacity || mb >= mrank_n || total > out_capacity) return 0;
    PCACC_BOUND(j, b_capacity);
    PCACC_BOUND(j, mrank_n);
    const int64_t d = accum_merge_dst(pos, mrank[j], total);
    if (d < 0) return 0;
    PCACC_BOUND(d, out_capacity);
    out_keys[d] = b_keys[j];
    for (int f = 0; f < ACC_FIELDS; ++f) out_acc[accum_field(f, d, out_capacity)] = b_acc[accum_field(f, j, b_capacity)];
    out_stamps[d] = b_stamps[j];
    out_stamps[out_capacity + d] = b_stamps[b_capacity + j];
    if (out_pierced) out_pierced[d] = b_pierced ? b_pierced[j] : 0;
    return ACCM_WRITTEN;
}

// ---- regrid ------------------------------------------------------------------------------------------------------------------------------------------
// Map row i under the pose T (12 doubles are read) on a grid of out_voxel_size: its key and term[ACC_FIELDS] = count, moving, count * q_x, count * q_y,
// count * q_z.  *count = the row's count (0 when i is no row).  false = unusable or invalid: *key and term then hold nothing.
PCACC_HD bool accg_row(const int64_t *acc, int64_t capacity, int64_t m, int64_t i, const double *T, double out_voxel_size, unsigned long long *key,
                       int64_t term[ACC_FIELDS], int64_t *count)
{
    *count = 0;
    if (i < 0 || i >= m || m > capacity) return false;
    PCACC_BOUND(i, capacity);
    const int64_t n = acc[accum_field(0, i, capacity)];
    *count = n;
    if (!(n > 0 && n <= ACCG_COUNT_MAX)) return false;
    const double c[3] = {accn_centroid(acc[accum_field(2, i, capacity)], n), accn_centroid(acc[accum_field(3, i, capacity)], n),
                         accn_centroid(acc[accum_field(4, i, capacity)], n)};
    int64_t q[3];
    if (!accum_point64(T, c, out_voxel_size, key, q)) return false;
    term[0] = n;
    term[1] = acc[accum_field(1, i, capacity)];
    for (int a = 0; a < 3; ++a) term[2 + a] = n * q[a];                           // n <= 2^31, |q| < 2^31
    return true;
}
