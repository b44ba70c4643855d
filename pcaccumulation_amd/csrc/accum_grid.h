// C4. The accumulated scene cloud (accum.hip): the per-point arithmetic (transform, validity, voxel key, fixed point), the index arithmetic of
// the window reduction, the search and the merge, and the extract formulas as __host__ __device__ functions, so that the SAME code runs in the
// kernels and in a g++ build (tests/accum_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.
//
// Per point (all float64, no FMA contraction, this operation order and no other):
//   w_a = ((r_a0 * x + r_a1 * y) + r_a2 * z) + t_a          rows 0-2 of a row-major 4x4
//   i_a = floor(w_a / voxel_size)                           one IEEE division
//   q_a = llrint(w_a * 65536)                               round to nearest, ties to even
// valid iff every w_a is finite, |w_a| < 32768 and -2^20 <= i_a < 2^20.  An invalid point is counted and contributes nothing: it is never
// clamped and never forms an address.
// Key: (i_x + 2^20) << 42 | (i_y + 2^20) << 21 | (i_z + 2^20) -- 63 bits, ascending keys = lexicographic (x, y, z); all ones = invalid.
#pragma once
#include "hd.h"

#define ACC_INVALID_KEY 0xffffffffffffffffull
#define ACC_IDX_BIAS 1048576            // 2^20 voxels either side of the origin, 21 bits per axis
#define ACC_COORD_LIMIT 32768.0         // |w| below this: q fits 32 bits, 2^31 points of one voxel still sum without overflow
#define ACC_FIXED_ONE 65536.0
#define ACC_FIELDS 5                    // count, moving, sum q_x, sum q_y, sum q_z -- field-major tables [ACC_FIELDS][capacity]

PCACC_HD unsigned long long accum_key(int64_t ix, int64_t iy, int64_t iz)  // every index in [-2^20, 2^20)
{
    return ((unsigned long long)(ix + ACC_IDX_BIAS) << 42) | ((unsigned long long)(iy + ACC_IDX_BIAS) << 21) | (unsigned long long)(iz + ACC_IDX_BIAS);
}

PCACC_HD void accum_unkey(unsigned long long key, int32_t c[3])
{
    c[0] = (int32_t)((key >> 42) & 0x1fffff) - ACC_IDX_BIAS;
    c[1] = (int32_t)((key >> 21) & 0x1fffff) - ACC_IDX_BIAS;
    c[2] = (int32_t)(key & 0x1fffff) - ACC_IDX_BIAS;
}

// Key and fixed-point coordinates of point p under the pose T (12 doubles are read); false = invalid, *key and q then hold nothing.
PCACC_HD bool accum_point(const double *T, const float *p, double voxel_size, unsigned long long *key, int64_t q[3])
{
    PCACC_NO_CONTRACT
    const double x = p[0], y = p[1], z = p[2];
    int64_t idx[3];
    for (int a = 0; a < 3; ++a) {
        const double w = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
        if (!pcacc_finite(w) || !(__builtin_fabs(w) < ACC_COORD_LIMIT)) return false;
        const double c = __builtin_floor(w / voxel_size);
        if (!(c >= -(double)ACC_IDX_BIAS && c < (double)ACC_IDX_BIAS)) return false;     // also false when w / voxel_size overflowed
        idx[a] = (int64_t)c;
        q[a] = (int64_t)__builtin_rint(w * ACC_FIXED_ONE);                                // |w * 65536| < 2^31: the cast is exact
    }
    *key = accum_key(idx[0], idx[1], idx[2]);
    return true;
}

// A row of the caller's point table named by the sort's value column: i itself when it lies in [0, n), else -1 (nothing is addressed).
PCACC_HD int64_t accum_point_index(int64_t i, int64_t n) { return (i >= 0 && i < n) ? i : -1; }

// First position in the ascending, duplicate-free keys[0..n) whose key is >= key: in [0, n].
PCACC_HD int64_t accum_lower_bound(const unsigned long long *keys, int64_t n, unsigned long long key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        PCACC_BOUND(mid, n);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Run (= window voxel) of sorted position i: `before` = run heads in front of i (exclusive scan), `head` = i is a head itself.
// In [0, runs), or -1 when the numbers do not fit (nothing is addressed then).
PCACC_HD int64_t accum_run_index(int64_t before, int64_t head, int64_t runs)
{
    const int64_t r = before + head - 1;
    return (r >= 0 && r < runs) ? r : -1;
}

// Merge of two ascending duplicate-free lists: the old entry at position p with `misses_before` new keys below it goes to p + misses_before;
// the new key that found `pos` old keys below it and is the `rank`-th new one goes to pos + rank.  Both in [0, total) or -1.
PCACC_HD int64_t accum_merge_dst(int64_t pos, int64_t shift, int64_t total)
{
    const int64_t d = pos + shift;
    return (pos >= 0 && shift >= 0 && d < total) ? d : -1;
}

// Element (field f, row i) of a field-major table of `capacity` rows.
PCACC_HD int64_t accum_field(int f, int64_t i, int64_t capacity)
{
    PCACC_BOUND(i, capacity);
    PCACC_BOUND(f, ACC_FIELDS);
    return (int64_t)f * capacity + i;
}

PCACC_HD bool accum_keep(int64_t count, int64_t moving, int64_t min_count, bool use_fraction, double max_moving_fraction)
{
    if (count < min_count || count <= 0) return false;
    if (use_fraction && !((double)moving / (double)count <= max_moving_fraction)) return false;
    return true;
}

PCACC_HD float accum_centroid(int64_t sum_q, int64_t count)
{
    PCACC_NO_CONTRACT
    return (float)(((double)sum_q / (double)count) * (1.0 / ACC_FIXED_ONE));
}
