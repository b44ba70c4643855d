// C5. Per-voxel surface normals of the accumulated scene cloud (accum_normals.hip; include/pcacc.h C5): the offset / range
// test, the neighbour row search and the whole result of one voxel as __host__ __device__ functions, so that the SAME code runs in the kernel and
// in a g++ build (tests/accum_normals_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction: both builds give the same bits.
//
// Voxel i = (x, y, z) of the participating set (dst[row] >= 0), radius r:
//   neighbours   every participating voxel with |delta|_inf <= r, itself included, visited in ASCENDING KEY ORDER: dx = -r..r, inside it dy = -r..r,
//                inside it the rows of the z run.  An offset that leaves [-2^20, 2^20) on an axis is skipped BEFORE a key is formed (x, y: the
//                column is skipped; z: the run is cut to the range) -- a key whose y or z field overflowed would alias another voxel.
//                One accum_lower_bound on key(x+dx, y+dy, z_lo) and a forward walk of at most 2r+1 rows while the key is <= key(x+dx, y+dy, z_hi).
//   c_a          ((double)sum q_a / (double)count) * 2^-16                                  the float64 centroid, not its float32 rounding
//   per visit    d = c_j - c_i (x, y, z);  S1_a += d_a;  then S2_xx += d_x d_x, S2_xy += d_x d_y, S2_xz += d_x d_z, S2_yy += d_y d_y,
//                S2_yz += d_y d_z, S2_zz += d_z d_z -- every sum starts at 0.0 and takes its terms in visiting order
//   mu_a         S1_a / k
//   C_ab         S2_ab / k - mu_a * mu_b   (a <= b, mirrored)
//   s, u         jacobi_svd3(C): s descending;  normal = u[:,2]
//   flags        1: k < min_neighbors;  2: s[1] <= SVD3_RANK_TOL * s[0];  either one: the normal is (0, 0, 0) and no sign rule runs
//   sign         t = t_first - stamp_base; with a viewpoint table and 0 <= t < S: e = viewpoint_t - c_i, flip iff (n_x e_x + n_y e_y) + n_z e_z < 0,
//                flag 4 set.  Otherwise: flip iff the first non-zero of (n_z, n_y, n_x) is negative (-0.0 is zero).
#pragma once
#include "accum_grid.h"
#include "svd3.h"

#define ACCN_MAX_RADIUS 3
#define ACCN_MIN_NEIGHBORS 3
#define ACCN_FEW_NEIGHBORS 1
#define ACCN_DEGENERATE 2
#define ACCN_VIEWPOINT 4

struct AccnResult {
    double normal[3];       // unit, or all zero when flags & 3
    double s[3];            // eigenvalues of the covariance, descending
    int k;                  // voxels visited
    int flags;
};

// i itself when it lies in [0, n), else -1 (nothing is addressed); the host build asserts.
PCACC_HD int64_t accn_index(int64_t i, int64_t n)
{
    PCACC_BOUND(i, n);
    return (i >= 0 && i < n) ? i : -1;
}

PCACC_HD bool accn_in_range(int64_t idx) { return idx >= -(int64_t)ACC_IDX_BIAS && idx < (int64_t)ACC_IDX_BIAS; }

PCACC_HD double accn_centroid(int64_t sum_q, int64_t count)
{
    PCACC_NO_CONTRACT
    return ((double)sum_q / (double)count) * (1.0 / ACC_FIXED_ONE);
}

// The z run of column (cx, cy) around cz: rows [*first, *first + n) of keys[0..m), n <= 2r+1 returned.  0 when the column lies outside the grid.
PCACC_HD int accn_column(const unsigned long long *keys, int64_t m, int64_t cx, int64_t cy, int64_t cz, int r, int64_t *first)
{
    *first = 0;
    if (!accn_in_range(cx) || !accn_in_range(cy)) return 0;
    const int64_t z_lo = cz - r < -(int64_t)ACC_IDX_BIAS ? -(int64_t)ACC_IDX_BIAS : cz - r;
    const int64_t z_hi = cz + r > (int64_t)ACC_IDX_BIAS - 1 ? (int64_t)ACC_IDX_BIAS - 1 : cz + r;
    if (z_lo > z_hi) return 0;
    const unsigned long long k_hi = accum_key(cx, cy, z_hi);
    const int64_t p0 = accum_lower_bound(keys, m, accum_key(cx, cy, z_lo));
    int n = 0;
    while (n < 2 * r + 1 && p0 + n < m) {
        const int64_t p = accn_index(p0 + n, m);
        if (p < 0 || keys[p] > k_hi) break;
        ++n;
    }
    *first = p0;
    return n;
}

// The whole result of map row i (a participating row: dst[i] >= 0).  dst[m]: output row of every map row, -1 = does not participate.
// false (and *out untouched, nothing addressed) when i is no row of the map.
PCACC_HD bool accum_normal_voxel(const unsigned long long *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, const int *dst,
                                 int64_t i, int radius, int min_neighbors, const double *viewpoints, int64_t n_viewpoints, int64_t stamp_base, AccnResult *out)
{
    PCACC_NO_CONTRACT
    if (accn_index(i, m) < 0 || m > capacity) return false;
    int32_t c[3];
    accum_unkey(keys[i], c);
    const int64_t cnt_i = acc[accum_field(0, i, capacity)];
    const double cx = accn_centroid(acc[accum_field(2, i, capacity)], cnt_i), cy = accn_centroid(acc[accum_field(3, i, capacity)], cnt_i),
                 cz = accn_centroid(acc[accum_field(4, i, capacity)], cnt_i);
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    int k = 0;
    for (int dx = -radius; dx <= radius; ++dx)
        for (int dy = -radius; dy <= radius; ++dy) {
            int64_t p0;
            const int n = accn_column(keys, m, (int64_t)c[0] + dx, (int64_t)c[1] + dy, c[2], radius, &p0);
            for (int e = 0; e < n; ++e) {
                const int64_t p = accn_index(p0 + e, m);
                if (p < 0 || dst[p] < 0) continue;
                const int64_t cnt = acc[accum_field(0, p, capacity)];
                const double ex = accn_centroid(acc[accum_field(2, p, capacity)], cnt) - cx, ey = accn_centroid(acc[accum_field(3, p, capacity)], cnt) - cy,
                             ez = accn_centroid(acc[accum_field(4, p, capacity)], cnt) - cz;
                s1x += ex; s1y += ey; s1z += ez;
                sxx += ex * ex; sxy += ex * ey; sxz += ex * ez; syy += ey * ey; syz += ey * ez; szz += ez * ez;
                ++k;
            }
        }
    const double kk = (double)k;                                        // k >= 1: the voxel visits itself
    const double mx = s1x / kk, my = s1y / kk, mz = s1z / kk;
    double C[3][3], u[3][3], s[3], v[3][3];
    C[0][0] = sxx / kk - mx * mx; C[0][1] = sxy / kk - mx * my; C[0][2] = sxz / kk - mx * mz;
    C[1][1] = syy / kk - my * my; C[1][2] = syz / kk - my * mz; C[2][2] = szz / kk - mz * mz;
    C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
    jacobi_svd3(C, u, s, v);
    int flags = 0;
    if (k < min_neighbors) flags |= ACCN_FEW_NEIGHBORS;
    if (s[1] <= SVD3_RANK_TOL * s[0]) flags |= ACCN_DEGENERATE;
    double nx = u[0][2], ny = u[1][2], nz = u[2][2];
    if (flags) {
        nx = ny = nz = 0.0;
    } else {
        const int64_t t = (int64_t)stamps[i] - stamp_base;                     // t_first: row 0 of stamps [2][capacity]
        bool flip;
        if (viewpoints && t >= 0 && t < n_viewpoints) {
            const int64_t row = accn_index(t, n_viewpoints);
            const double ex = viewpoints[3 * row] - cx, ey = viewpoints[3 * row + 1] - cy, ez = viewpoints[3 * row + 2] - cz;
            flip = (nx * ex + ny * ey) + nz * ez < 0.0;
            flags |= ACCN_VIEWPOINT;
        } else {
            flip = nz != 0.0 ? nz < 0.0 : (ny != 0.0 ? ny < 0.0 : nx < 0.0);
        }
        if (flip) { nx = 0.0 - nx; ny = 0.0 - ny; nz = 0.0 - nz; }            // a zero component stays +0.0
    }
    out->normal[0] = nx; out->normal[1] = ny; out->normal[2] = nz;
    out->s[0] = s[0]; out->s[1] = s[1]; out->s[2] = s[2];
    out->k = k;
    out->flags = flags;
    return true;
}
