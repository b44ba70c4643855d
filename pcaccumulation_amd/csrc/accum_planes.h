// C18. Planar segments of the accumulated scene cloud by normal-gated region growing (accum_planes.hip; include/pcacc.h C18):
// which rows take part, the rule that joins two of them, the integer moments of a segment and the plane fitted to them, as __host__ __device__
// functions, so that the SAME code runs in the kernels and in a g++ build (tests/accum_planes_host_driver.cpp) where every table index is
// assert-checked before anything runs on a GPU.  Includes nothing of HIP; calls accum_unkey, accum_field, accn_index, accn_column (through
// accc_edges), accn_centroid, accc_* of accum_components.h, uf_* of union_find.h and jacobi_svd3, and restates none of them.
//
//   rows        extract row j takes part iff the filter keeps it, the mask (if any) is non-zero at j, flags[j] has neither FEW_NEIGHBORS nor
//               DEGENERATE, and (double)e2 <= max_variation * (((double)e0 + (double)e1) + (double)e2) with e = eigenvalues[j]: a product, no
//               division.  The first test that fails names the counter.  The result is the byte table part[kept], which serves accc_takes_part /
//               accc_row / accc_edges as their mask: the neighbour search is C11's, not a second one.
//   edges       accc_edges reports every pair (i, p < i) of rows that take part with |delta|_inf <= radius, once; acpl_joined decides it, float64, no
//               FMA contraction:  |(n_ix n_px + n_iy n_py) + n_iz n_pz| >= cos_angle;  d = c_p - c_i (accn_centroid);
//               |(n_ix d_x + n_iy d_y) + n_iz d_z| <= max_offset;  the same with n_p.  Symmetric in (i, p) bit for bit: products commute and
//               c_i - c_p is the exact negation.  So the segments are the components of a graph that is a function of the records and the given
//               normals, and labels (C11's numbering by smallest row) depend on no order.
//   pass 1      C11's integer reductions (accc_stat_row / accc_stat_merge) and D = max over members and axes of |u_a - A_a|, u = floor(sum q / count)
//               the integer centroid of a row, A = u of the segment's first row.
//   shift       the smallest s >= 0 with t = (D >> s) + 1 <= 2^31 and t t <= 2^62 / voxels: |e| <= t below, so no sum of pass 2 leaves int64.
//   pass 2      e_a = (u_a - A_a) >> s (arithmetic);  S1_a += e_a;  S2_ab += e_a e_b (xx, xy, xz, yy, yz, zz): integers, any order.
//   fit         mu_a = S1_a / voxels;  C_ab = S2_ab / voxels - mu_a mu_b;  jacobi_svd3;  scale = 2^(s - 16);  normal = u[:,2] with C5's sign rule
//               without a viewpoint;  eigenvalues = s_k (scale scale);  centroid = (A_a + mu_a 2^s) 2^-16;  offset = (n_x c_x + n_y c_y) + n_z c_z;
//               mse = s_2 (scale scale).  s_1 <= SVD3_RANK_TOL s_0: ACPL_PLANE_DEGENERATE, normal, offset and mse 0.0.
//   distance    of a row to the plane of its own segment: ((n_x c_x + n_y c_y) + n_z c_z) - offset; 0.0 without a segment or a plane.
#pragma once
#include "accum_components.h"

#define ACPL_COUNTERS 9
#define ACPL_C_ROWS 0
#define ACPL_C_PARTICIPATING 1
#define ACPL_C_OUTSIDE 2
#define ACPL_C_MASKED 3
#define ACPL_C_INVALID 4
#define ACPL_C_NOT_FLAT 5
#define ACPL_C_SEGMENTS 6
#define ACPL_C_LARGEST 7
#define ACPL_C_STATUS 8
#define ACPL_OK 0
#define ACPL_BAD_ROWS 1
#define ACPL_GAVE_UP 2
#define ACPL_PLANE_DEGENERATE 1
#define ACPL_TAKES_PART 0                // acpl_class
#define ACPL_OUTSIDE (-1)
#define ACPL_MASKED (-2)
#define ACPL_INVALID (-3)
#define ACPL_NOT_FLAT (-4)
#define ACPL_MAX_SHIFT 32

// The normal tables have one row per kept row, and so has the mask when there is one.
PCACC_HD bool acpl_rows_fit(const uint8_t *mask, int64_t mask_rows, int64_t n_rows, int64_t kept) { return n_rows == kept && accc_mask_fits(mask, mask_rows, kept); }

PCACC_HD bool acpl_flat(float e0, float e1, float e2, double max_variation)
{
    PCACC_NO_CONTRACT
    return (double)e2 <= max_variation * (((double)e0 + (double)e1) + (double)e2);           // NaN: not flat
}

// Extract row j (the tables have been found to fit): ACPL_TAKES_PART or the first test it fails.
PCACC_HD int acpl_class(const uint8_t *mask, const uint8_t *flags, const float *eigenvalues, int64_t kept, int64_t j, double max_variation)
{
    if (accn_index(j, kept) < 0) return ACPL_OUTSIDE;
    if (mask != nullptr && mask[j] == 0) return ACPL_MASKED;
    if ((flags[j] & (ACCN_FEW_NEIGHBORS | ACCN_DEGENERATE)) != 0) return ACPL_INVALID;
    if (!acpl_flat(eigenvalues[3 * j], eigenvalues[3 * j + 1], eigenvalues[3 * j + 2], max_variation)) return ACPL_NOT_FLAT;
    return ACPL_TAKES_PART;
}

// What the rule reads of one row: the given normal of extract row j and the float64 centroid of map row i.
struct AcplRow {
    double nx, ny, nz, cx, cy, cz;
};

PCACC_HD bool acpl_row(const int64_t *acc, int64_t capacity, int64_t m, int64_t i, const float *normals, int64_t kept, int64_t j, AcplRow *r)
{
    if (accn_index(i, m) < 0 || accn_index(j, kept) < 0 || m > capacity) return false;
    const int64_t count = acc[accum_field(0, i, capacity)];
    if (count <= 0) return false;
    r->nx = (double)normals[3 * j]; r->ny = (double)normals[3 * j + 1]; r->nz = (double)normals[3 * j + 2];
    r->cx = accn_centroid(acc[accum_field(2, i, capacity)], count);
    r->cy = accn_centroid(acc[accum_field(3, i, capacity)], count);
    r->cz = accn_centroid(acc[accum_field(4, i, capacity)], count);
    return true;
}

PCACC_HD bool acpl_joined(const AcplRow &a, const AcplRow &b, double cos_angle, double max_offset)
{
    PCACC_NO_CONTRACT
    const double dot = (a.nx * b.nx + a.ny * b.ny) + a.nz * b.nz;
    if (!(__builtin_fabs(dot) >= cos_angle)) return false;
    const double dx = b.cx - a.cx, dy = b.cy - a.cy, dz = b.cz - a.cz;
    const double off_a = (a.nx * dx + a.ny * dy) + a.nz * dz;
    if (!(__builtin_fabs(off_a) <= max_offset)) return false;
    const double off_b = (b.nx * dx + b.ny * dy) + b.nz * dz;
    return __builtin_fabs(off_b) <= max_offset;
}

// floor(a / b), b > 0
PCACC_HD int64_t acpl_floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The integer centroid of map row i, in units of 2^-16 m; false (nothing addressed) when i is no row of the map or holds no point.
PCACC_HD bool acpl_int_centroid(const int64_t *acc, int64_t capacity, int64_t m, int64_t i, int64_t *ux, int64_t *uy, int64_t *uz)
{
    if (i < 0 || i >= m || m > capacity) return false;
    PCACC_BOUND(i, capacity);
    const int64_t count = acc[accum_field(0, i, capacity)];
    if (count <= 0) return false;
    *ux = acpl_floor_div(acc[accum_field(2, i, capacity)], count);
    *uy = acpl_floor_div(acc[accum_field(3, i, capacity)], count);
    *uz = acpl_floor_div(acc[accum_field(4, i, capacity)], count);
    return true;
}

PCACC_HD uint64_t acpl_abs_diff(int64_t u, int64_t a) { return u >= a ? (uint64_t)u - (uint64_t)a : (uint64_t)a - (uint64_t)u; }

// max over the axes of |u - A|: below 2^32, both being below 2^31 in magnitude.
PCACC_HD uint64_t acpl_spread(int64_t ux, int64_t uy, int64_t uz, int32_t ax, int32_t ay, int32_t az)
{
    uint64_t d = acpl_abs_diff(ux, ax);
    const uint64_t dy = acpl_abs_diff(uy, ay), dz = acpl_abs_diff(uz, az);
    d = dy > d ? dy : d;
    return dz > d ? dz : d;
}

// The smallest s with t = (D >> s) + 1 <= 2^31 and t t <= 2^62 / voxels.  voxels in [1, 2^31): s = 32 (t = 1) always passes.
PCACC_HD int acpl_shift(uint64_t spread, int64_t voxels)
{
    const uint64_t room = ((uint64_t)1 << 62) / (uint64_t)(voxels > 0 ? voxels : 1);
    for (int s = 0; s < ACPL_MAX_SHIFT; ++s) {
        const uint64_t t = (spread >> s) + 1;
        if (t <= ((uint64_t)1 << 31) && t * t <= room) return s;
    }
    return ACPL_MAX_SHIFT;
}

// What one row, or a run of rows of one segment, adds to the sums of pass 2.  Named scalars: nothing here is indexed at run time.
struct AcplMoments {
    int64_t x, y, z, xx, xy, xz, yy, yz, zz;
};

PCACC_HD void acpl_moments_none(AcplMoments *q) { q->x = q->y = q->z = q->xx = q->xy = q->xz = q->yy = q->yz = q->zz = 0; }

// |u - A| <= D and s = acpl_shift(D, voxels): |e| <= (D >> s) + 1.  A shift count outside [0, 32] adds nothing.
PCACC_HD void acpl_moments_row(int64_t ux, int64_t uy, int64_t uz, int32_t ax, int32_t ay, int32_t az, int s, AcplMoments *q)
{
    acpl_moments_none(q);
    if (s < 0 || s > ACPL_MAX_SHIFT) return;
    const int64_t ex = (ux - ax) >> s, ey = (uy - ay) >> s, ez = (uz - az) >> s;
    q->x = ex; q->y = ey; q->z = ez;
    q->xx = ex * ex; q->xy = ex * ey; q->xz = ex * ez; q->yy = ey * ey; q->yz = ey * ez; q->zz = ez * ez;
}

PCACC_HD void acpl_moments_merge(AcplMoments *a, const AcplMoments &b)
{
    a->x += b.x; a->y += b.y; a->z += b.z;
    a->xx += b.xx; a->xy += b.xy; a->xz += b.xz; a->yy += b.yy; a->yz += b.yz; a->zz += b.zz;
}

struct AcplFit {
    double normal[3], eigenvalues[3], centroid[3], offset, mse;
    int flags;
};

PCACC_HD double acpl_pow2(int e)                                                             // 2^e, |e| <= 64, exact
{
    double v = 1.0;
    for (int k = 0; k < e; ++k) v = v * 2.0;
    for (int k = 0; k > e; --k) v = v * 0.5;
    return v;
}

// The plane of one segment from its integer moments: a fixed sequence of float64 operations.  s1 [3], s2 [6] (xx, xy, xz, yy, yz, zz), anchor [3].
PCACC_HD void acpl_fit(const int32_t *anchor, int s, int64_t voxels, const int64_t *s1, const int64_t *s2, AcplFit *out)
{
    PCACC_NO_CONTRACT
    const double n = (double)(voxels > 0 ? voxels : 1);
    const double mx = (double)s1[0] / n, my = (double)s1[1] / n, mz = (double)s1[2] / n;
    double C[3][3], u[3][3], sv[3], v[3][3];
    C[0][0] = (double)s2[0] / n - mx * mx; C[0][1] = (double)s2[1] / n - mx * my; C[0][2] = (double)s2[2] / n - mx * mz;
    C[1][1] = (double)s2[3] / n - my * my; C[1][2] = (double)s2[4] / n - my * mz; C[2][2] = (double)s2[5] / n - mz * mz;
    C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
    jacobi_svd3(C, u, sv, v);
    const double scale = acpl_pow2(s - 16), scale2 = scale * scale, step = acpl_pow2(s);
    out->eigenvalues[0] = sv[0] * scale2; out->eigenvalues[1] = sv[1] * scale2; out->eigenvalues[2] = sv[2] * scale2;
    out->centroid[0] = ((double)anchor[0] + mx * step) * (1.0 / ACC_FIXED_ONE);
    out->centroid[1] = ((double)anchor[1] + my * step) * (1.0 / ACC_FIXED_ONE);
    out->centroid[2] = ((double)anchor[2] + mz * step) * (1.0 / ACC_FIXED_ONE);
    out->flags = 0;
    if (sv[1] <= SVD3_RANK_TOL * sv[0]) {                                                    // fewer than three voxels that are not collinear
        out->flags = ACPL_PLANE_DEGENERATE;
        out->normal[0] = out->normal[1] = out->normal[2] = 0.0;
        out->offset = 0.0;
        out->mse = 0.0;
        return;
    }
    double nx = u[0][2], ny = u[1][2], nz = u[2][2];
    const bool flip = nz != 0.0 ? nz < 0.0 : (ny != 0.0 ? ny < 0.0 : nx < 0.0);             // C5's rule without a viewpoint
    if (flip) { nx = 0.0 - nx; ny = 0.0 - ny; nz = 0.0 - nz; }
    out->normal[0] = nx; out->normal[1] = ny; out->normal[2] = nz;
    out->offset = (nx * out->centroid[0] + ny * out->centroid[1]) + nz * out->centroid[2];
    out->mse = sv[2] * scale2;
}

// The signed distance of map row i to a plane.
PCACC_HD double acpl_distance(const int64_t *acc, int64_t capacity, int64_t m, int64_t i, double nx, double ny, double nz, double offset)
{
    PCACC_NO_CONTRACT
    if (accn_index(i, m) < 0 || m > capacity) return 0.0;
    const int64_t count = acc[accum_field(0, i, capacity)];
    if (count <= 0) return 0.0;
    const double cx = accn_centroid(acc[accum_field(2, i, capacity)], count), cy = accn_centroid(acc[accum_field(3, i, capacity)], count),
                 cz = accn_centroid(acc[accum_field(4, i, capacity)], count);
    return ((nx * cx + ny * cy) + nz * cz) - offset;
}
