// C9. Looking a scan's points up in the accumulated scene cloud (accum_query.hip; include/pcacc.h C9): for every point of a scan
// its own voxel's record, the nearest kept centroid among the 27 voxels around it and the distance to that voxel's plane, as __host__ __device__
// functions, so that the SAME code runs in the kernel and in a g++ build (tests/accum_query_host_driver.cpp) where every table index is assert-checked
// before anything runs on a GPU.  Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in the order written here.
// Nothing of C4 - C6 is restated: accr_world, accr_match, accr_candidate, accn_centroid, accum_lower_bound, accum_field, accn_index, accum_keep are called.
//
// Per point p under the pose T (rows 0-2 of a row-major 4x4):
//   world      accr_world(T, p, voxel_size, w, idx); false: INVALID, every other output at its default.  Never clamped, no key, no address.
//   own voxel  the map row whose key is key(idx) among the first m rows (one accum_lower_bound): OCCUPIED; count, moving, t_first, t_last copied; pierced
//              from the sidecar (0 without one); KEPT iff accum_keep(count, moving, min_count, use_fraction, max_moving_fraction).  No row: all 0.
//   nearest    accr_match with max_d2 = max_distance * max_distance: the kept rows (dst[row] >= 0) of the 3 x 3 x 3 voxels around idx in ascending key
//              order, d2 = (e_x e_x + e_y e_y) + e_z e_z against the float64 centroid, strict < (ties to the lowest key), accepted iff d2 <= max_d2.
//              require_normal: a candidate must also have a normal without flag 1 or 2 (C6's candidate set); otherwise accr_candidate gets a NULL flag
//              table and every kept row is a candidate.  MATCHED: row = dst[best] (extract's row), nearest = (float)centroid, distance = sqrt(d2).
//   plane      with normal tables and neither flag 1 nor 2 on the matched row: NORMAL, plane_distance = (n_x e_x + n_y e_y) + n_z e_z, n the widened
//              float32 normal, e = w - c: accr_terms' r, signed.
//   defaults   row = -1, nearest = 0, distance = plane_distance = +inf: a threshold distance < x never admits an unmatched point.
// Normal tables whose n_rows differs from the rows the filter keeps (BAD_TABLE): no normal table is addressed and no point is MATCHED; world and own
// voxel are reported as always.
//
// How far the 27 voxels reach.  A centroid is the mean of fixed-point values that each lie within 2^-17 m of a point inside the voxel, so it lies within
// 2^-17 m of the voxel itself.  A point's own voxel is the centre of the 27, so any voxel outside them is at least voxel_size away from the point, and a
// centroid outside them is farther than voxel_size - 2^-17.  For max_distance <= 0.9 voxel_size (voxel sizes of 1e-4 m and up: 0.1 voxel_size >= 1e-5 >
// 2^-17) no such centroid can be accepted, so the match IS the global nearest kept centroid within max_distance.  At max_distance = voxel_size the
// 27-voxel search itself is the contract, as in C6.
#pragma once
#include "accum_register.h"

#define ACCQ_INVALID 1
#define ACCQ_OCCUPIED 2
#define ACCQ_KEPT 4
#define ACCQ_MATCHED 8
#define ACCQ_NORMAL 16

#define ACCQ_COUNTERS 7               // points, invalid, occupied, kept, matched, normal, BAD_TABLE (0 / 1)
#define ACCQ_C_POINTS 0
#define ACCQ_C_INVALID 1
#define ACCQ_C_OCCUPIED 2
#define ACCQ_C_KEPT 3
#define ACCQ_C_MATCHED 4
#define ACCQ_C_NORMAL 5
#define ACCQ_C_BAD_TABLE 6

#define ACCQ_NO_TABLES 0              // accq_tables: no normal tables were given
#define ACCQ_TABLES 1                 // they have the rows the filter keeps
#define ACCQ_BAD_TABLES (-1)          // they do not: nothing of them is addressed, nothing matches

struct AccqParams {                   // named scalars: nothing here is indexed at run time
    const unsigned long long *keys;   // [capacity]           | the first m rows of a map
    const int64_t *acc;               // [ACC_FIELDS][capacity]
    const int32_t *stamps;            // [2][capacity]
    const int32_t *pierced;           // [capacity] or NULL
    const int *dst;                   // [m]: extract's row of every map row, -1 = filtered out
    const float *normals;             // [n_rows][3] or NULL
    const uint8_t *flags;             // [n_rows] or NULL
    int64_t capacity, m, n_rows, min_count;
    double voxel_size, max_d2, max_moving_fraction;
    int use_fraction, require_normal;
};

struct AccqRecord {                   // everything one point is told
    int64_t count, moving;
    double distance, plane_distance;
    float nearest_x, nearest_y, nearest_z;
    int32_t t_first, t_last, pierced, row;
    int status;
};

struct AccqOut {                      // field-major columns of n rows; nearest is [n][3]
    uint8_t *status;
    int64_t *count, *moving;
    int32_t *t_first, *t_last, *pierced, *row;
    float *nearest;
    double *distance, *plane_distance;
};

// What the normal tables are worth: kept = the rows the filter keeps (pass 1 of C5).
PCACC_HD int accq_tables(bool given, int64_t kept, int64_t n_rows)
{
    if (!given) return ACCQ_NO_TABLES;
    return kept == n_rows ? ACCQ_TABLES : ACCQ_BAD_TABLES;
}

// The whole answer for point p; tables = accq_tables(...).
PCACC_HD void accq_point(const AccqParams &P, int tables, const double *T, const float *p, AccqRecord *r)
{
    PCACC_NO_CONTRACT
    r->count = r->moving = 0;
    r->distance = r->plane_distance = __builtin_inf();
    r->nearest_x = r->nearest_y = r->nearest_z = 0.0f;
    r->t_first = r->t_last = r->pierced = 0;
    r->row = -1;
    r->status = 0;
    double w[3], c[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
    int64_t idx[3], row = -1;
    if (!accr_world(T, p, P.voxel_size, w, idx)) { r->status = ACCQ_INVALID; return; }
    if (P.m > P.capacity) return;                                                            // tables that do not fit address nothing
    int status = 0;
    const unsigned long long key = accum_key(idx[0], idx[1], idx[2]);
    const int64_t q = accum_lower_bound(P.keys, P.m, key);                                   // in [0, m]
    if (q < P.m) {
        const int64_t o = accn_index(q, P.m);
        if (o >= 0 && P.keys[o] == key) {
            PCACC_BOUND(o, P.capacity);
            r->count = P.acc[accum_field(0, o, P.capacity)];
            r->moving = P.acc[accum_field(1, o, P.capacity)];
            r->t_first = P.stamps[o];
            r->t_last = P.stamps[P.capacity + o];
            r->pierced = P.pierced ? P.pierced[o] : 0;
            status |= ACCQ_OCCUPIED;
            if (accum_keep(r->count, r->moving, P.min_count, P.use_fraction != 0, P.max_moving_fraction)) status |= ACCQ_KEPT;
        }
    }
    r->status = status;
    if (tables == ACCQ_BAD_TABLES) return;
    const uint8_t *need = (P.require_normal && tables == ACCQ_TABLES) ? P.flags : (const uint8_t *)0;
    if (accr_match(P.keys, P.acc, P.capacity, P.m, P.dst, need, P.n_rows, w, idx, P.max_d2, &row, c, &d2) < 0) return;
    status |= ACCQ_MATCHED;
    r->row = (int32_t)row;
    r->nearest_x = (float)c[0]; r->nearest_y = (float)c[1]; r->nearest_z = (float)c[2];
    r->distance = __builtin_sqrt(d2);
    if (tables == ACCQ_TABLES) {
        const int64_t j = accn_index(row, P.n_rows);
        if (j >= 0 && !(P.flags[j] & (ACCN_FEW_NEIGHBORS | ACCN_DEGENERATE))) {
            const double nx = P.normals[3 * j], ny = P.normals[3 * j + 1], nz = P.normals[3 * j + 2];
            const double ex = w[0] - c[0], ey = w[1] - c[1], ez = w[2] - c[2];
            r->plane_distance = (nx * ex + ny * ey) + nz * ez;
            status |= ACCQ_NORMAL;
        }
    }
    r->status = status;
}

// Row i of every output column, each written once.  false (nothing addressed) when i is no row.
PCACC_HD bool accq_store(const AccqOut &o, int64_t i, int64_t n, const AccqRecord &r)
{
    if (accn_index(i, n) < 0) return false;
    o.status[i] = (uint8_t)r.status;
    o.count[i] = r.count;
    o.moving[i] = r.moving;
    o.t_first[i] = r.t_first;
    o.t_last[i] = r.t_last;
    o.pierced[i] = r.pierced;
    o.row[i] = r.row;
    o.nearest[3 * i] = r.nearest_x; o.nearest[3 * i + 1] = r.nearest_y; o.nearest[3 * i + 2] = r.nearest_z;
    o.distance[i] = r.distance;
    o.plane_distance[i] = r.plane_distance;
    return true;
}
