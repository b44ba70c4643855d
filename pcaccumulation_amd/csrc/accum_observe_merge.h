// C15. Two tables of observed space into one, and a table under a rigid pose and / or a new voxel size (accum_observe_merge.hip; include/pcacc.h C15,
// DESIGN.md section 9o): the move of a row of either table to its row of the union, the decision of a merge with its state words, and the key, the run
// and the fold of a table row that is re-voxelised, as __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build
// (tests/accum_observe_merge_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.  Includes nothing of HIP.
//
// merge   A (ma rows) and B (mb rows), both ascending and duplicate-free, on ONE grid.  B row j is searched in A by accm_search (accum_merge.h); mrank =
//         exclusive scan of the misses.  A row p -> row p + mrank[accum_lower_bound(B, key)] of the union: rays a + b, stamps min / max when B holds the
//         key, else copied; missed B row j -> row position + mrank[j], copied.
//         rays is an int64 sum with no clamp.  A ray count is the number of walked rays that visited the voxel, so it is at most the WALKED word of its
//         table; WALKED grows by at most 2^30 per observe call and a merge adds two WALKED words, so 2^63 takes 2^33 calls or as many doublings by
//         self-merge as nobody runs (62).  The sum of two counts is bounded by the sum of the two WALKED words, which the state carries beside it.
// regrid  a row is its voxel's CENTRE: p_a = (float64(c_a) + 0.5) * in_voxel_size, then accum_point64 (accum_merge.h: C4's transform, validity rule,
//         floor(w_a / out_voxel_size) and key, float64, no FMA contraction).  Rows that land on one key fold to rays = MAX, t_first = min, t_last = max.
//         MAX and not C12's sum: a ray that crossed k source voxels of one destination voxel is ONE ray, the sum would count it k times, and overstating
//         the evidence for "free" is the unsafe direction.  For a nested coarsening the maximum is a lower bound on the rays that crossed the coarse
//         voxel; under a rotation it is an estimate.  A row whose centre is invalid (C4: not finite, |w_a| >= 32768 or an index outside [-2^20, 2^20))
//         is never clamped and forms no address.
//
// Where every index comes from, each behind a PCACC_BOUND:
//   table positions     accum_lower_bound (accm_search, accom_old_row), used only after p < m
//   destinations        accum_merge_dst (accom_old_row, accom_new_row), used only after the decision gave `total` <= out_capacity
//   sorted positions    accum_point_index on the sort's value column; run indices from accum_run_index (accog_position)
//   ma, mb, m           used only after the launcher checked them against the capacity, and accom_decide / accog_begin against the state words
#pragma once
#include "accum_observe.h"
#include "accum_merge.h"

// the state words of a table (include/pcacc.h PCACC_OBSERVE_*; accum_observe_merge.hip static_asserts the values)
#define ACCOM_STATE_WORDS 16
#define ACCOM_NUM_VOXELS 0
#define ACCOM_STATUS 1
#define ACCOM_NEEDED 2
#define ACCOM_NEEDED_VISITS 3
#define ACCOM_CALL_VISITS 4
#define ACCOM_CALL_VOXELS 5
#define ACCOM_WALKED 6                  // .. ACCOM_WALKED + 4: walked, dropped, skipped, truncated, visits
// counters of a merge and of a regrid (include/pcacc.h PCACC_OBSERVED_MERGE_*, PCACC_OBSERVED_REGRID_*)
#define ACCOM_C_STATUS 0
#define ACCOM_C_NEEDED 1
#define ACCOM_C_SHARED 2
#define ACCOM_C_NEW 3
#define ACCOG_C_ROWS_IN 0
#define ACCOG_C_ROWS_OUT 1
#define ACCOG_C_DROPPED_ROWS 2

// ---- merge -------------------------------------------------------------------------------------------------------------------------------------------
// The state words describe the tables the caller handed in.
PCACC_HD bool accom_state_fits(const int64_t *state, int64_t ma, const int64_t *b_state, int64_t mb)
{
    return state[ACCOM_NUM_VOXELS] == ma && b_state[ACCOM_NUM_VOXELS] == mb;
}

// The one decision of a merge: `fresh` = keys of B that A lacks.  Writes the four counters; on OK the state words of the result into `state` (B's words
// are read before any word of `state` is written: state and b_state may be the same words).  -> the status; only ACCO_OK lets a table be written.
PCACC_HD int accom_decide(bool bad_state, int64_t ma, int64_t mb, int64_t fresh, int64_t out_capacity, const int64_t *b_state, int64_t *state,
                          int64_t *counters)
{
    if (bad_state) {
        counters[ACCOM_C_STATUS] = ACCO_BAD_STATE;
        counters[ACCOM_C_NEEDED] = counters[ACCOM_C_SHARED] = counters[ACCOM_C_NEW] = 0;
        return ACCO_BAD_STATE;
    }
    const int64_t total = ma + fresh;
    counters[ACCOM_C_NEEDED] = total;
    counters[ACCOM_C_SHARED] = mb - fresh;
    counters[ACCOM_C_NEW] = fresh;
    const int status = acco_decide_rows(total, out_capacity);
    counters[ACCOM_C_STATUS] = status;
    if (status != ACCO_OK) return status;
    int64_t b[5];
    for (int k = 0; k < 5; ++k) b[k] = b_state[ACCOM_WALKED + k];
    state[ACCOM_NUM_VOXELS] = total;
    state[ACCOM_STATUS] = ACCO_OK;
    state[ACCOM_NEEDED] = total;
    state[ACCOM_NEEDED_VISITS] = state[ACCOM_CALL_VISITS] = state[ACCOM_CALL_VOXELS] = 0;      // a merge walks nothing
    for (int k = 0; k < 5; ++k) state[ACCOM_WALKED + k] += b[k];
    return status;
}

// A row p to its row of the union; mrank has mrank_n >= mb + 1 entries.  -> the destination row, or -1 when p is no row or the destination does not
// fit (nothing is addressed then).  *shared = 1 when B holds the key.
PCACC_HD int64_t accom_old_row(const unsigned long long *a_keys, const int64_t *a_rays, const int32_t *a_stamps, int64_t a_capacity, int64_t ma,
                               const unsigned long long *b_keys, const int64_t *b_rays, const int32_t *b_stamps, int64_t b_capacity, int64_t mb,
                               const int *mrank, int64_t mrank_n, int64_t p, unsigned long long *out_keys, int64_t *out_rays, int32_t *out_stamps,
                               int64_t out_capacity, int64_t total, int *shared)
{
    *shared = 0;
    if (p < 0 || p >= ma || ma > a_capacity || mb > b_capacity || mb >= mrank_n || total > out_capacity) return -1;
    PCACC_BOUND(p, a_capacity);
    const unsigned long long key = a_keys[p];
    const int64_t j = accum_lower_bound(b_keys, mb, key);                        // in [0, mb]
    PCACC_BOUND(j, mrank_n);
    const int64_t d = accum_merge_dst(p, mrank[j], total);
    if (d < 0) return -1;
    PCACC_BOUND(d, out_capacity);
    const bool hit = j < mb && b_keys[j] == key;
    const int32_t t0 = a_stamps[p], t1 = a_stamps[a_capacity + p];
    out_keys[d] = key;
    if (hit) {
        PCACC_BOUND(j, b_capacity);
        const int32_t u0 = b_stamps[j], u1 = b_stamps[b_capacity + j];
        out_rays[d] = a_rays[p] + b_rays[j];
        out_stamps[d] = u0 < t0 ? u0 : t0;
        out_stamps[out_capacity + d] = u1 > t1 ? u1 : t1;
        *shared = 1;
    } else {                                                                     // a key of one table only: copied bit for bit
        out_rays[d] = a_rays[p];
        out_stamps[d] = t0;
        out_stamps[out_capacity + d] = t1;
    }
    return d;
}

// Missed B row j (A lacks its key, pos A keys below it) to row pos + mrank[j] of the union, copied.  -> the destination row or -1 (nothing addressed).
PCACC_HD int64_t accom_new_row(const unsigned long long *b_keys, const int64_t *b_rays, const int32_t *b_stamps, int64_t b_capacity, int64_t mb,
                               const int *mrank, int64_t mrank_n, int64_t j, int64_t pos, unsigned long long *out_keys, int64_t *out_rays,
                               int32_t *out_stamps, int64_t out_capacity, int64_t total)
{
    if (j < 0 || j >= mb || mb > b_capacity || mb >= mrank_n || total > out_capacity) return -1;
    PCACC_BOUND(j, b_capacity);
    PCACC_BOUND(j, mrank_n);
    const int64_t d = accum_merge_dst(pos, mrank[j], total);
    if (d < 0) return -1;
    PCACC_BOUND(d, out_capacity);
    out_keys[d] = b_keys[j];
    out_rays[d] = b_rays[j];
    out_stamps[d] = b_stamps[j];
    out_stamps[out_capacity + d] = b_stamps[b_capacity + j];
    return d;
}

// ---- regrid ------------------------------------------------------------------------------------------------------------------------------------------
// Table row i under the pose T (12 doubles are read), from a grid of in_voxel_size onto one of out_voxel_size: the key of the voxel its centre lands in.
// false = i is no row, or the centre is invalid: *key then holds nothing.
PCACC_HD bool accog_row(const unsigned long long *keys, int64_t capacity, int64_t m, int64_t i, const double *T, double in_voxel_size,
                        double out_voxel_size, unsigned long long *key)
{
    PCACC_NO_CONTRACT
    if (i < 0 || i >= m || m > capacity) return false;
    PCACC_BOUND(i, capacity);
    int32_t c[3];
    accum_unkey(keys[i], c);
    const double p[3] = {((double)c[0] + 0.5) * in_voxel_size, ((double)c[1] + 0.5) * in_voxel_size, ((double)c[2] + 0.5) * in_voxel_size};
    int64_t q[3];
    return accum_point64(T, p, out_voxel_size, key, q);
}

// Sorted position i of m starts a run (= a row of the new table); the invalid key, which sorts to the end, starts none.
PCACC_HD int accog_head(const unsigned long long *sorted, int64_t i, int64_t m)
{
    if (i < 0 || i >= m) return 0;
    PCACC_BOUND(i, m);
    const unsigned long long k = sorted[i];
    return (k != ACC_INVALID_KEY && (i == 0 || sorted[i - 1] != k)) ? 1 : 0;
}

// Sorted position i: the run it belongs to (vox = exclusive scan of the heads) and, in *row, the input row the sort's value column names.
// -> the run in [0, runs), or -1 when the position holds the invalid key or the numbers do not fit (nothing is addressed then).
PCACC_HD int64_t accog_position(const unsigned long long *sorted, const int *idx, const int *head, const int *vox, int64_t m, int64_t runs, int64_t i,
                                int64_t *row)
{
    *row = -1;
    if (i < 0 || i >= m) return -1;
    PCACC_BOUND(i, m);
    if (sorted[i] == ACC_INVALID_KEY) return -1;
    const int64_t r = accum_point_index(idx[i], m);
    if (r < 0) return -1;
    PCACC_BOUND(r, m);
    *row = r;
    return accum_run_index(vox[i], head[i], runs);
}

// The fold of two sources of one destination voxel.
PCACC_HD void accog_fold(int64_t *rays, int32_t *t_first, int32_t *t_last, int64_t r, int32_t a, int32_t b)
{
    if (r > *rays) *rays = r;
    if (a < *t_first) *t_first = a;
    if (b > *t_last) *t_last = b;
}

// The state words of the new table: the rows, the five cumulative counters of the input, the rest 0.  The counters describe the RAYS the input table was
// given, which a regrid does not walk again: VISITS no longer equals the sum of `rays` (rows fold by maximum, and dropped rows take theirs along).
PCACC_HD void accog_state(const int64_t *in_state, int64_t rows_out, int64_t *out_state)
{
    int64_t c[5];
    for (int k = 0; k < 5; ++k) c[k] = in_state[ACCOM_WALKED + k];
    for (int k = 0; k < ACCOM_STATE_WORDS; ++k) out_state[k] = 0;
    out_state[ACCOM_NUM_VOXELS] = rows_out;
    for (int k = 0; k < 5; ++k) out_state[ACCOM_WALKED + k] = c[k];
}
