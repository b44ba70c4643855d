// C13. Two accumulated scene clouds compared, and the rows of extract() that a mask names as a new map (accum_compare.hip; include/pcacc.h C13,
// DESIGN.md section 9m): the whole answer for one row of one map against the other map, its store, the select flag of a map row and nothing else, as
// __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build (tests/accum_compare_host_driver.cpp) where every table
// index is assert-checked before anything runs on a GPU.  Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in
// the order written here.  Nothing of C4 - C12 is restated: accum_unkey, accum_lower_bound, accum_field, accn_index, accn_centroid, accr_match and
// accr_move_row are called.
//
// compare  maps A and B on ONE grid, both ascending and duplicate-free, each with its row table dst (extract's row of every map row, -1 = filtered
//          out) under one filter.  Per own row i with dst_own[i] >= 0, against the other map O:
//   own      key = keys[i]; idx = accum_unkey(key); w_a = accn_centroid(sum q_a, count): the float64 centroid of C5
//   same     q = accum_lower_bound(O.keys, O.m, key); HELD iff q < O.m and O.keys[q] == key; pierced = O's ray count of row q (0 without a sidecar, 0
//            without HELD); SAME iff HELD and O.dst[q] >= 0; same_row = O.dst[q] (O's extract row), else -1
//   nearest  accr_match(O.keys, O.acc, O.capacity, O.m, O.dst, NULL, O.kept, w, idx, max_distance^2): C9's call, C6's search.  A hit: NEAR, row = O's
//            extract row, distance = sqrt(d2).  How far the 27 voxels reach is argued in accum_query.h: for max_distance <= 0.9 voxel_size the hit is
//            the nearest kept centroid of the whole of O.
//   defaults same_row = row = -1, distance = +inf, pierced = 0
//          The record goes to row dst_own[i] of the own side's columns: one output row per row of extract(), in its order.
// select   map row i is selected iff dst[i] >= 0 and (mask[dst[i]] != 0) != invert.  A mask whose mask_rows differs from the rows the filter keeps
//          (BAD_MASK) selects nothing and none of its entries is addressed.  A selected row moves with accr_move_row: bit for bit.
#pragma once
#include "accum_prune.h"
#include "accum_query.h"

#define ACCD_SAME 1                   // the other map holds this voxel and its filter keeps it
#define ACCD_HELD 2                   // the other map holds this voxel
#define ACCD_NEAR 4                   // a kept centroid of the other map lies within max_distance

#define ACCD_SIDE_COUNTERS 6          // per side, A then B
#define ACCD_COUNTERS 12
#define ACCD_C_ROWS 0
#define ACCD_C_KEPT 1
#define ACCD_C_SAME 2
#define ACCD_C_HELD 3
#define ACCD_C_NEAR 4
#define ACCD_C_ONLY 5                 // kept rows with neither SAME nor NEAR

#define ACCS_COUNTERS 4
#define ACCS_C_STATUS 0
#define ACCS_C_ROWS 1
#define ACCS_C_KEPT 2
#define ACCS_C_SELECTED 3
#define ACCS_OK 0
#define ACCS_BAD_MASK 1

struct AccdMap {                      // the first m rows of one map with its row table; named scalars: nothing here is indexed at run time
    const unsigned long long *keys;   // [capacity]
    const int64_t *acc;               // [ACC_FIELDS][capacity]
    const int32_t *pierced;           // [capacity] or NULL
    const int *dst;                   // [m]: extract's row of every map row, -1 = filtered out
    int64_t capacity, m, kept;        // kept: the rows the filter keeps
};

struct AccdRecord {                   // everything one row is told
    double distance;
    int32_t same_row, row, pierced;
    int status;
};

struct AccdOut {                      // columns of one side, [m] each, the first kept rows written
    uint8_t *status;
    int32_t *same_row, *row, *pierced;
    double *distance;
};

// The whole answer for row i of `own` against `other`.  false (r at its defaults, nothing addressed) when i is no row of own or a table does not fit.
PCACC_HD bool accd_row(const AccdMap &own, const AccdMap &other, int64_t i, double max_d2, AccdRecord *r)
{
    PCACC_NO_CONTRACT
    r->distance = __builtin_inf();
    r->same_row = r->row = -1;
    r->pierced = 0;
    r->status = 0;
    if (accn_index(i, own.m) < 0 || own.m > own.capacity || other.m > other.capacity) return false;
    const unsigned long long key = own.keys[i];
    int32_t c[3];
    accum_unkey(key, c);
    const int64_t idx[3] = {c[0], c[1], c[2]};
    const int64_t cnt = own.acc[accum_field(0, i, own.capacity)];
    const double w[3] = {accn_centroid(own.acc[accum_field(2, i, own.capacity)], cnt), accn_centroid(own.acc[accum_field(3, i, own.capacity)], cnt),
                         accn_centroid(own.acc[accum_field(4, i, own.capacity)], cnt)};
    int status = 0;
    const int64_t q = accum_lower_bound(other.keys, other.m, key);                            // in [0, other.m]
    if (q < other.m) {
        const int64_t o = accn_index(q, other.m);
        if (o >= 0 && other.keys[o] == key) {
            PCACC_BOUND(o, other.capacity);
            status |= ACCD_HELD;
            r->pierced = other.pierced ? other.pierced[o] : 0;
            const int j = other.dst[o];
            if (j >= 0) { status |= ACCD_SAME; r->same_row = j; }
        }
    }
    int64_t row = -1;
    double centroid[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
    if (accr_match(other.keys, other.acc, other.capacity, other.m, other.dst, (const uint8_t *)0, other.kept, w, idx, max_d2, &row, centroid, &d2) >= 0) {
        status |= ACCD_NEAR;
        r->row = (int32_t)row;
        r->distance = __builtin_sqrt(d2);
    }
    r->status = status;
    return true;
}

// Row d of every column of one side, each written once.  false (nothing addressed) when d is no row the filter keeps or the columns do not hold them.
PCACC_HD bool accd_store(const AccdOut &o, int64_t d, int64_t kept, int64_t m, const AccdRecord &r)
{
    if (d < 0 || d >= kept || kept > m) return false;
    PCACC_BOUND(d, m);
    o.status[d] = (uint8_t)r.status;
    o.same_row[d] = r.same_row;
    o.row[d] = r.row;
    o.pierced[d] = r.pierced;
    o.distance[d] = r.distance;
    return true;
}

// ---- select ------------------------------------------------------------------------------------------------------------------------------------------
PCACC_HD int accs_status(int64_t kept, int64_t mask_rows) { return kept == mask_rows ? ACCS_OK : ACCS_BAD_MASK; }

// 1 iff map row i is selected; status = accs_status(...).  BAD_MASK: 0, and neither dst nor mask is addressed.
PCACC_HD int accs_selected(const int *dst, int64_t m, const uint8_t *mask, int64_t mask_rows, int status, int invert, int64_t i)
{
    if (status != ACCS_OK || i < 0 || i >= m) return 0;
    PCACC_BOUND(i, m);
    const int64_t j = dst[i];
    if (j < 0 || accn_index(j, mask_rows) < 0) return 0;
    return ((mask[j] != 0) != (invert != 0)) ? 1 : 0;
}
