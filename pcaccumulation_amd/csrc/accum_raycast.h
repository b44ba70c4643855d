// C10. Casting rays into the accumulated scene cloud (accum_raycast.hip; include/pcacc.h C10): looking from an origin towards a
// target, the first voxel the map keeps and how far away it is, as __host__ __device__ functions, so that the SAME code runs in the kernel and in a g++
// build (tests/accum_raycast_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in the order written here.
// Nothing of C4 - C9 is restated: accp_end_point, accp_origin_index, accp_in_range (inside accp_step, the step C7 walks with), accum_key,
// accum_lower_bound, accum_field, accn_index and accn_centroid are called.
//
// Ray i: target p (float32, row i of targets [n,3]) and origin = row origin_index[i] of origins [S,3] (float64), both in the caller's frame: C7's inputs.
//   end points   o = pose . origin, e = pose . p through accp_end_point.  DROPPED when origin_index[i] lies outside [0, S) or o / e fails C4's validity
//                rule.  Never clamped, no key, no address.
//   extent       d = e - o, L = sqrt((d_x^2 + d_y^2) + d_z^2), t_start = min_range / L.  With a max_range t_end = max_range / L (the ray may run past its
//                target), without one t_end = 1 - margin / L (the ray runs to its target: C7's formula).  !(L > 0), !(t_end > 0) or !(t_start < t_end):
//                SKIPPED.
//   walk         C7's, bit for bit: the start voxel floor(o_a / voxel_size) with t_in = 0, then accp_step per step (b_a and t_a afresh, strict <, ties x, y,
//                z; !(t_best < t_end) or an index that leaves [-2^20, 2^20) ends the walk; the entered voxel has t_in = t_best).  A walk that would make
//                visit number max_steps + 1 ends instead: TRUNCATED.
//   visit        visits += 1.  The voxel is a candidate iff !(t_in < t_start); a voxel that is none is walked without a search.  For a candidate
//                pos = accum_lower_bound(keys, m, key); HIT iff pos < m, keys[pos] == key and dst[pos] >= 0 (dst: the row table of the filter, as C9 gets
//                it).  The walk stops at the first HIT.
//   outputs      status (MISS 0, HIT 1, TRUNCATED 2, SKIPPED 3, DROPPED 4); row = dst[pos], extract's row under the same filter; coords = the hit voxel;
//                point = (float)c, c the float64 centroid (extract's row); range_in = t_in * L; depth = (((c_x - o_x) d_x + (c_y - o_y) d_y) + (c_z - o_z)
//                d_z) / L; length = L (0 for DROPPED, whatever L was for SKIPPED); visits.
//   defaults     without a HIT row = -1, coords = point = 0, range_in = depth = +inf: a threshold depth < x never admits a miss.
//
// depth against range_in.  The ray enters the hit voxel at range_in, and along a unit direction no two points of a cube of side voxel_size lie more than
// sqrt(3) voxel_size apart.  The centroid is the mean of fixed-point values that each lie within 2^-17 m of a point inside the voxel, so it lies within
// 2^-17 m of the voxel itself.  Hence |depth - range_in| <= sqrt(3) voxel_size + 2^-17, plus the rounding of the few operations above (below 1e-9 m for
// |w| < 32768).
#pragma once
#include "accum_normals.h"
#include "accum_pierce.h"

#define ACCY_MAX_STEPS ACCP_MAX_STEPS

#define ACCY_MISS 0
#define ACCY_HIT 1
#define ACCY_TRUNCATED 2
#define ACCY_SKIPPED 3
#define ACCY_DROPPED 4

#define ACCY_COUNTERS 7               // rays, dropped, skipped, hit, missed, truncated, visits: the first is the sum of the next five
#define ACCY_C_RAYS 0
#define ACCY_C_DROPPED 1
#define ACCY_C_SKIPPED 2
#define ACCY_C_HIT 3
#define ACCY_C_MISSED 4
#define ACCY_C_TRUNCATED 5
#define ACCY_C_VISITS 6

struct AccyParams {                   // named scalars: nothing here is indexed at run time
    const unsigned long long *keys;   // [capacity]           | the first m rows of a map
    const int64_t *acc;               // [ACC_FIELDS][capacity]
    const int *dst;                   // [m]: extract's row of every map row, -1 = filtered out
    int64_t capacity, m;
    double voxel_size, min_range, margin, max_range;
    int use_range, max_steps;
};

struct AccyRecord {                   // everything one ray is told
    double range_in, depth, length;
    float point_x, point_y, point_z;
    int32_t row, coord_x, coord_y, coord_z, visits;
    int status;
};

struct AccyOut {                      // columns of n rows; coords and point are [n][3]
    uint8_t *status;
    int32_t *row, *coords;
    float *point;
    double *range_in, *depth, *length;
    int32_t *visits;
};

// The whole of one ray.  T: 12 doubles of the pose; p: the target; origin: its row of the origin table, read only when origin_ok.
PCACC_HD void accy_ray(const AccyParams &P, const double *T, const float *p, const double *origin, bool origin_ok, AccyRecord *r)
{
    PCACC_NO_CONTRACT
    r->range_in = r->depth = __builtin_inf();
    r->length = 0.0;
    r->point_x = r->point_y = r->point_z = 0.0f;
    r->row = -1;
    r->coord_x = r->coord_y = r->coord_z = 0;
    r->visits = 0;
    r->status = ACCY_DROPPED;
    double e[3], o[3];
    int64_t ie[3], i[3];
    if (!origin_ok || P.m > P.capacity) return;                                  // tables that do not fit address nothing
    if (!accp_end_point(T, origin[0], origin[1], origin[2], P.voxel_size, o, i)) return;
    if (!accp_end_point(T, (double)p[0], (double)p[1], (double)p[2], P.voxel_size, e, ie)) return;
    r->status = ACCY_SKIPPED;
    const double dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
    const double L = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    r->length = L;
    if (!(L > 0.0)) return;
    const double t_start = P.min_range / L;
    const double t_end = P.use_range ? P.max_range / L : 1.0 - P.margin / L;
    if (!(t_end > 0.0) || !(t_start < t_end)) return;
    r->status = ACCY_MISS;
    const double d[3] = {dx, dy, dz};
    double t_in = 0.0;
    int visits = 0;
    for (;;) {
        ++visits;
        if (!(t_in < t_start)) {
            const unsigned long long key = accum_key(i[0], i[1], i[2]);
            const int64_t pos = accum_lower_bound(P.keys, P.m, key);             // in [0, m]; m = 0: no load
            if (pos < P.m) {
                const int64_t q = accn_index(pos, P.m);
                if (q >= 0 && P.keys[q] == key && P.dst[q] >= 0) {
                    const int64_t count = P.acc[accum_field(0, q, P.capacity)];
                    const double cx = accn_centroid(P.acc[accum_field(2, q, P.capacity)], count);
                    const double cy = accn_centroid(P.acc[accum_field(3, q, P.capacity)], count);
                    const double cz = accn_centroid(P.acc[accum_field(4, q, P.capacity)], count);
                    r->status = ACCY_HIT;
                    r->row = (int32_t)P.dst[q];
                    r->coord_x = (int32_t)i[0]; r->coord_y = (int32_t)i[1]; r->coord_z = (int32_t)i[2];
                    r->point_x = (float)cx; r->point_y = (float)cy; r->point_z = (float)cz;
                    r->range_in = t_in * L;
                    r->depth = (((cx - o[0]) * dx + (cy - o[1]) * dy) + (cz - o[2]) * dz) / L;
                    break;
                }
            }
        }
        if (!accp_step(o, d, P.voxel_size, t_end, i, &t_in)) break;
        if (visits >= P.max_steps) { r->status = ACCY_TRUNCATED; break; }
    }
    r->visits = (int32_t)visits;
}

// Row i of every output column, each written once.  false (nothing addressed) when i is no row.
PCACC_HD bool accy_store(const AccyOut &o, int64_t i, int64_t n, const AccyRecord &r)
{
    if (accn_index(i, n) < 0) return false;
    o.status[i] = (uint8_t)r.status;
    o.row[i] = r.row;
    o.coords[3 * i] = r.coord_x; o.coords[3 * i + 1] = r.coord_y; o.coords[3 * i + 2] = r.coord_z;
    o.point[3 * i] = r.point_x; o.point[3 * i + 1] = r.point_y; o.point[3 * i + 2] = r.point_z;
    o.range_in[i] = r.range_in;
    o.depth[i] = r.depth;
    o.length[i] = r.length;
    o.visits[i] = r.visits;
    return true;
}
