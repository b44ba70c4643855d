// C7. Rays through the accumulated scene cloud (accum_pierce.hip; include/pcacc.h C7): the end points, the eligibility rule, the
// voxel walk and the row lookup of one ray as __host__ __device__ functions, so that the SAME code runs in the kernel and in a g++ build
// (tests/accum_pierce_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction: both builds give the same integers.
//
// Ray i: scan point p (float32) and origin = row origin_index[i] of origins [S,3] (float64), both in the scan frame.
//   end points   e = pose . p, o = pose . origin with C4's order ((r0 x + r1 y) + r2 z) + t.  DROPPED when origin_index[i] lies outside [0, S), or a
//                coordinate w of o or e is not finite, has |w| >= 32768, or floor(w / voxel_size) leaves [-2^20, 2^20).  Never clamped, no key, no address.
//   eligibility  (after the drop rule) a point flagged moving is SKIPPED.  d = e - o, L = sqrt((d_x^2 + d_y^2) + d_z^2), t_end = 1 - margin / L, with a
//                max_range t_end = min(t_end, max_range / L).  !(L > 0) or !(t_end > 0): SKIPPED.  Every other ray is WALKED.
//   walk         i_a = floor(o_a / voxel_size).  Visit i.  For every axis with d_a != 0: b_a = double(i_a + (d_a > 0 ? 1 : 0)) * voxel_size,
//                t_a = (b_a - o_a) / d_a -- afresh at every step, nothing is carried from step to step.  The smallest t_a by strict < (ties: x, y, z).
//                !(t_a < t_end): the walk ends.  Otherwise i_a +-= 1; an index that leaves [-2^20, 2^20) ends the walk.  A walk that would make visit
//                number max_steps + 1 ends instead and the ray is TRUNCATED; the visits made so far stay.
//   visit        key = accum_key(i), pos = accum_lower_bound(keys, m, key).  On a hit, and with a stamp s only when t_last < s or t_first > s (the voxel
//                was not being filled at time s), pierced[pos] += 1 and hits += 1.  Rows are not filtered by count or moving fraction.
#pragma once
#include "accum_grid.h"

#define ACCP_MAX_STEPS 65536
#define ACCP_WALKED 0
#define ACCP_DROPPED 1
#define ACCP_SKIPPED 2

struct AccpRay {
    int status;             // ACCP_WALKED / ACCP_DROPPED / ACCP_SKIPPED
    int truncated;          // 1: cut at max_steps visits
    int visits;             // voxels visited
    int hits;               // visits that added to a row
};

PCACC_HD bool accp_in_range(int64_t idx) { return idx >= -(int64_t)ACC_IDX_BIAS && idx < (int64_t)ACC_IDX_BIAS; }

// A row of the origin table: i itself when it lies in [0, n), else -1 (nothing is addressed).
PCACC_HD int64_t accp_origin_index(int64_t i, int64_t n) { return (i >= 0 && i < n) ? i : -1; }

// w = T . (x, y, z) in C4's order and the voxel indices of w; false = C4's validity rule fails, w and idx then hold nothing.
PCACC_HD bool accp_end_point(const double *T, double x, double y, double z, double voxel_size, double w[3], int64_t idx[3])
{
    PCACC_NO_CONTRACT
    for (int a = 0; a < 3; ++a) {
        w[a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
        if (!pcacc_finite(w[a]) || !(__builtin_fabs(w[a]) < ACC_COORD_LIMIT)) return false;
        const double c = __builtin_floor(w[a] / voxel_size);
        if (!(c >= -(double)ACC_IDX_BIAS && c < (double)ACC_IDX_BIAS)) return false;
        idx[a] = (int64_t)c;
    }
    return true;
}

// One step of the walk, the choice C7 and C10 (accum_raycast.h) share: for every axis with d_a != 0 the plane b_a and t_a = (b_a - o_a) / d_a afresh, the
// smallest t_a by strict < (ties: x, y, z).  false: the walk ends -- no axis, !(t_best < t_end), or the moved index left [-2^20, 2^20) (i has moved then).
// true: i moved by one voxel along the winning axis and the ray enters that voxel at *t_in = t_best.
PCACC_HD bool accp_step(const double o[3], const double d[3], double voxel_size, double t_end, int64_t i[3], double *t_in)
{
    PCACC_NO_CONTRACT
    int best = -1;
    double t_best = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0) continue;
        const double b = (double)(i[a] + (d[a] > 0.0 ? 1 : 0)) * voxel_size;
        const double t = (b - o[a]) / d[a];
        if (best < 0 || t < t_best) { best = a; t_best = t; }
    }
    if (best < 0 || !(t_best < t_end)) return false;
    bool inside = true;
    for (int a = 0; a < 3; ++a)                                                  // no run-time index into i: the three stay in registers
        if (a == best) { i[a] += d[a] > 0.0 ? 1 : -1; inside = accp_in_range(i[a]); }
    *t_in = t_best;
    return inside;
}

// The whole of one ray.  T: 12 doubles of the pose; p: the scan point; origin: its row of the origin table, read only when origin_ok (origin_index in range);
// stamps [2][capacity]; t_end's max_range is used when use_range.  hit(pos) is called for every counted visit, pos in [0, m): the kernel adds with an
// integer atomic, the host build with ++.
template <class Hit>
PCACC_HD AccpRay accp_ray(const double *T, const float *p, const double *origin, bool origin_ok, bool moving, double voxel_size, double margin, bool use_range,
                          double max_range, bool use_stamp, int32_t stamp, int max_steps, const unsigned long long *keys, const int32_t *stamps,
                          int64_t capacity, int64_t m, Hit &hit)
{
    PCACC_NO_CONTRACT
    AccpRay r;
    r.status = ACCP_DROPPED; r.truncated = 0; r.visits = 0; r.hits = 0;
    double e[3], o[3];
    int64_t ie[3], i[3];
    if (!origin_ok || m > capacity) return r;
    if (!accp_end_point(T, origin[0], origin[1], origin[2], voxel_size, o, i)) return r;
    if (!accp_end_point(T, (double)p[0], (double)p[1], (double)p[2], voxel_size, e, ie)) return r;
    r.status = ACCP_SKIPPED;
    if (moving) return r;
    const double dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
    const double L = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(L > 0.0)) return r;
    double t_end = 1.0 - margin / L;
    if (use_range) {
        const double t_range = max_range / L;
        if (t_range < t_end) t_end = t_range;
    }
    if (!(t_end > 0.0)) return r;
    r.status = ACCP_WALKED;
    const double d[3] = {dx, dy, dz};
    double t_in = 0.0;
    for (;;) {
        const unsigned long long key = accum_key(i[0], i[1], i[2]);
        const int64_t pos = accum_lower_bound(keys, m, key);                     // in [0, m]; m = 0: no load
        ++r.visits;
        if (pos < m) {
            PCACC_BOUND(pos, m);
            if (keys[pos] == key && (!use_stamp || stamps[capacity + pos] < stamp || stamps[pos] > stamp)) { hit(pos); ++r.hits; }
        }
        if (!accp_step(o, d, voxel_size, t_end, i, &t_in)) break;
        if (r.visits >= max_steps) { r.truncated = 1; break; }
    }
    return r;
}
