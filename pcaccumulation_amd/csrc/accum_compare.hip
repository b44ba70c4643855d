// C13. Two accumulated scene clouds compared in both directions, and the rows of extract() that a mask names as a new map (include/pcacc.h C13,
// DESIGN.md section 9m).
//
//   compare  rows     pass 1 of C5 (accn_rows_launch) on A and on B: dst[m], extract's row of every map row, rows[kept] its inverse; both kept counts
//                     stay on the device.  A side without rows launches nothing.
//            side     ONE kernel, launched once per side with the two maps swapped: one lane per row the filter keeps, consecutive lanes on
//                     consecutive extract rows (their searches in the other map's ascending keys land next to each other, as in accq_point_kernel):
//                     accd_row of accum_compare.h -- the code the host build runs with every index assert-checked -- then accd_store: every column
//                     as the coalesced column it is, every row written once by the lane of its row.  The four counts are summed per lane, reduced
//                     over the wave, one integer atomic per wave and non-zero counter.
//   select   rows     pass 1 of C5
//            flags    one lane per map row: accs_selected; the kernel compares the kept count with mask_rows itself (BAD_MASK)
//            scan     scan.h over the flags -> the destination of every selected row
//            move     accr_move_row of C8, every destination written once; one thread writes the counters and the eight state words
// Neither entry reads anything back.  No floating-point atomics, no LDS beyond the scan's, no inline assembly.  Every result is an integer, a copied
// record or a float64 computed in one order: two runs give the same bits.
#include "scan.h"
#include "accum_compare.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCD_BLOCK 256

static_assert(ACCD_SAME == PCACC_COMPARE_SAME && ACCD_HELD == PCACC_COMPARE_HELD && ACCD_NEAR == PCACC_COMPARE_NEAR &&
              ACCD_COUNTERS == PCACC_COMPARE_COUNTERS && ACCD_SIDE_COUNTERS == PCACC_COMPARE_SIDE_COUNTERS && ACCD_C_ROWS == PCACC_COMPARE_ROWS &&
              ACCD_C_KEPT == PCACC_COMPARE_KEPT && ACCD_C_SAME == PCACC_COMPARE_N_SAME && ACCD_C_HELD == PCACC_COMPARE_N_HELD &&
              ACCD_C_NEAR == PCACC_COMPARE_N_NEAR && ACCD_C_ONLY == PCACC_COMPARE_N_ONLY && ACCS_COUNTERS == PCACC_SELECT_COUNTERS &&
              ACCS_C_STATUS == PCACC_SELECT_STATUS && ACCS_C_ROWS == PCACC_SELECT_ROWS && ACCS_C_KEPT == PCACC_SELECT_KEPT &&
              ACCS_C_SELECTED == PCACC_SELECT_SELECTED && ACCS_OK == PCACC_SELECT_OK && ACCS_BAD_MASK == PCACC_SELECT_BAD_MASK,
              "accum_compare.h and include/pcacc.h name the same bits and counters");

// ---- compare -----------------------------------------------------------------------------------------------------------------------------------------
// One side: `own` against `other`.  own.m >= 1; other.m may be 0 (its tables are then never addressed).  counters: the six words of this side.
static __global__ __launch_bounds__(ACCD_BLOCK) void accd_side_kernel(AccdMap own, AccdMap other, const int *__restrict__ own_rows,
                                                                       const int64_t *__restrict__ own_kept, const int64_t *__restrict__ other_kept,
                                                                       double max_d2, AccdOut out, unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    int64_t kept = *own_kept;                                                                // uniform over the grid
    if (kept > own.m) kept = own.m;
    if (kept < 0) kept = 0;
    own.kept = kept;
    other.kept = other_kept ? *other_kept : 0;
    long long c_same = 0, c_held = 0, c_near = 0, c_only = 0;
    for (int64_t j = (int64_t)blockIdx.x * ACCD_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCD_BLOCK) {
        const int64_t i = own_rows[j];
        if (i < 0 || i >= own.m || own.dst[i] != j) continue;                                // a table that does not fit addresses nothing
        AccdRecord r;
        if (!accd_row(own, other, i, max_d2, &r)) continue;
        accd_store(out, j, kept, own.m, r);
        c_same += (r.status & ACCD_SAME) != 0; c_held += (r.status & ACCD_HELD) != 0; c_near += (r.status & ACCD_NEAR) != 0;
        c_only += (r.status & (ACCD_SAME | ACCD_NEAR)) == 0;
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACCD_C_SAME, c_same);
    accum_wave_count(counters, ACCD_C_HELD, c_held);
    accum_wave_count(counters, ACCD_C_NEAR, c_near);
    accum_wave_count(counters, ACCD_C_ONLY, c_only);
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                               // the memset left 0; no lane adds to these two
        counters[ACCD_C_ROWS] = (unsigned long long)own.m;
        counters[ACCD_C_KEPT] = (unsigned long long)kept;
    }
}

struct AccdWs { AccnRowsWs a, b; };

static size_t accd_carve(int64_t ma, int64_t mb, AccdWs *w, char *base)
{
    const size_t off = accn_rows_ws_carve(ma, &w->a, base);
    return off + accn_rows_ws_carve(mb, &w->b, base + off);
}

extern "C" int pcacc_accum_compare_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes)
{
    if (!bytes || ma < 0 || ma > ACCUM_MAX_CAPACITY || mb < 0 || mb > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccdWs w;
    *bytes = accd_carve(ma, mb, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_compare(const int64_t *a_keys, const int64_t *a_acc, const int32_t *a_pierced, int64_t a_capacity, int64_t ma,
                                   const int64_t *b_keys, const int64_t *b_acc, const int32_t *b_pierced, int64_t b_capacity, int64_t mb,
                                   double voxel_size, double max_distance, int64_t min_count, int32_t use_fraction, double max_moving_fraction,
                                   uint8_t *out_a_status, int32_t *out_a_same_row, int32_t *out_a_row, double *out_a_distance,
                                   int32_t *out_a_pierced, uint8_t *out_b_status, int32_t *out_b_same_row, int32_t *out_b_row,
                                   double *out_b_distance, int32_t *out_b_pierced, int64_t *counters, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    if (a_capacity < 0 || a_capacity > ACCUM_MAX_CAPACITY || b_capacity < 0 || b_capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (ma < 0 || ma > a_capacity || mb < 0 || mb > b_capacity || min_count < 1 || !counters) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0) || !(max_distance > 0.0) || !(max_distance <= voxel_size)) return PCACC_E_ARG;
    if (ma > 0 && (!a_keys || !a_acc || !out_a_status || !out_a_same_row || !out_a_row || !out_a_distance || !out_a_pierced)) return PCACC_E_ARG;
    if (mb > 0 && (!b_keys || !b_acc || !out_b_status || !out_b_same_row || !out_b_row || !out_b_distance || !out_b_pierced)) return PCACC_E_ARG;
    AccdWs w;
    if (ma > 0 || mb > 0) {
        if (!workspace) return PCACC_E_ARG;
        if (workspace_bytes < accd_carve(ma, mb, &w, (char *)workspace)) return PCACC_E_WORKSPACE;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCD_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (ma == 0 && mb == 0) return PCACC_OK;
    if (ma > 0 && accn_rows_launch(a_acc, a_capacity, ma, min_count, (int)use_fraction, max_moving_fraction, w.a.rows, w.a.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    if (mb > 0 && accn_rows_launch(b_acc, b_capacity, mb, min_count, (int)use_fraction, max_moving_fraction, w.b.rows, w.b.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    AccdMap A, B;
    A.keys = (const unsigned long long *)a_keys; A.acc = a_acc; A.pierced = a_pierced; A.dst = ma > 0 ? w.a.rows.dst : (const int *)nullptr;
    A.capacity = a_capacity; A.m = ma; A.kept = 0;
    B.keys = (const unsigned long long *)b_keys; B.acc = b_acc; B.pierced = b_pierced; B.dst = mb > 0 ? w.b.rows.dst : (const int *)nullptr;
    B.capacity = b_capacity; B.m = mb; B.kept = 0;
    const int64_t *kept_a = ma > 0 ? (const int64_t *)w.a.kept : (const int64_t *)nullptr;
    const int64_t *kept_b = mb > 0 ? (const int64_t *)w.b.kept : (const int64_t *)nullptr;
    const double max_d2 = max_distance * max_distance;
    const AccdOut out_a = {out_a_status, out_a_same_row, out_a_row, out_a_pierced, out_a_distance};
    const AccdOut out_b = {out_b_status, out_b_same_row, out_b_row, out_b_pierced, out_b_distance};
    unsigned long long *c = (unsigned long long *)counters;
    // a lane runs ten serial searches: many small workgroups spread over the CUs, as accum_query.hip
    if (ma > 0)
        hipLaunchKernelGGL(accd_side_kernel, dim3(pcacc_grid(ma, ACCD_BLOCK, 1 << 22)), dim3(ACCD_BLOCK), 0, st, A, B, (const int *)w.a.rows.rows, kept_a,
                           kept_b, max_d2, out_a, c);
    if (mb > 0)
        hipLaunchKernelGGL(accd_side_kernel, dim3(pcacc_grid(mb, ACCD_BLOCK, 1 << 22)), dim3(ACCD_BLOCK), 0, st, B, A, (const int *)w.b.rows.rows, kept_b,
                           kept_a, max_d2, out_b, c + ACCD_SIDE_COUNTERS);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// ---- select ------------------------------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(ACCD_BLOCK) void accs_flag_kernel(const int *__restrict__ dst, int64_t m, const int64_t *__restrict__ kept_ptr,
                                                                       const uint8_t *__restrict__ mask, int64_t mask_rows, int invert,
                                                                       int *__restrict__ flag)
{
    const int status = accs_status(*kept_ptr, mask_rows);                                    // uniform over the grid
    for (int64_t i = (int64_t)blockIdx.x * ACCD_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCD_BLOCK)
        flag[i] = accs_selected(dst, m, mask, mask_rows, status, invert, i);
}

// kept_ptr, flag, spos = NULL: an empty map (m = 0).  A BAD_MASK writes the counters and nothing else.
static __global__ __launch_bounds__(ACCD_BLOCK) void accs_move_kernel(const unsigned long long *__restrict__ in_keys, const int64_t *__restrict__ in_acc,
                                                                       const int32_t *__restrict__ in_stamps, const int32_t *__restrict__ in_pierced,
                                                                       int64_t in_capacity, int64_t m, const int64_t *__restrict__ kept_ptr,
                                                                       int64_t mask_rows, const int *__restrict__ flag, const int *__restrict__ spos,
                                                                       unsigned long long *__restrict__ out_keys, int64_t *__restrict__ out_acc,
                                                                       int32_t *__restrict__ out_stamps, int32_t *__restrict__ out_pierced,
                                                                       int64_t out_capacity, int64_t *__restrict__ counters, int64_t *__restrict__ state)
{
    const int64_t kept = kept_ptr ? *kept_ptr : 0;
    const int status = accs_status(kept, mask_rows);
    const int64_t selected = (spos && status == ACCS_OK) ? spos[m] : 0;
    if (status == ACCS_OK)
        for (int64_t i = (int64_t)blockIdx.x * ACCD_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCD_BLOCK) {
            if (!flag[i]) continue;
            accr_move_row(in_keys, in_acc, in_stamps, in_pierced, in_capacity, m, i, out_keys, out_acc, out_stamps, out_pierced, out_capacity, selected,
                          accum_merge_dst(spos[i], 0, selected));
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counters[ACCS_C_STATUS] = status;
        counters[ACCS_C_ROWS] = m;
        counters[ACCS_C_KEPT] = kept;
        counters[ACCS_C_SELECTED] = selected;
        if (status == ACCS_OK) {
            for (int k = 0; k < PCACC_ACCUM_STATE_WORDS; ++k) state[k] = 0;
            state[PCACC_ACCUM_NUM_VOXELS] = selected;
        }
    }
}

struct AccsWs : AccnRowsWs { int *flag, *spos, *chunk; };

static size_t accs_carve(AccsWs *w, char *base, int64_t m)                                   // m >= 1
{
    size_t off = accn_rows_ws_carve(m, w, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->flag = (int *)take((size_t)m * 4);
    w->spos = (int *)take((size_t)(m + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    return off;
}

extern "C" int pcacc_accum_select_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccsWs w;
    *bytes = accs_carve(&w, nullptr, m > 0 ? m : 1);
    return PCACC_OK;
}

extern "C" int pcacc_accum_select(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                                  int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction, const uint8_t *mask, int64_t mask_rows,
                                  int32_t invert, int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity,
                                  int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || in_capacity < m || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < m || out_capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (min_count < 1 || mask_rows < 0 || (mask_rows > 0 && !mask) || !counters || !state) return PCACC_E_ARG;
    if (m > 0 && (!in_keys || !in_acc || !in_stamps || !out_keys || !out_acc || !out_stamps || (in_pierced && !out_pierced) || !workspace)) return PCACC_E_ARG;
    if (accum_tables_overlap(in_keys, in_acc, in_stamps, in_pierced, in_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity)) return PCACC_E_ARG;
    AccsWs w;
    if (m > 0 && workspace_bytes < accs_carve(&w, (char *)workspace, m)) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    const unsigned long long *keys = (const unsigned long long *)in_keys;
    int32_t *op = in_pierced ? out_pierced : (int32_t *)nullptr;
    if (m == 0) {
        hipLaunchKernelGGL(accs_move_kernel, dim3(1), dim3(ACCD_BLOCK), 0, st, keys, in_acc, in_stamps, in_pierced, in_capacity, m, (const int64_t *)nullptr,
                           mask_rows, (const int *)nullptr, (const int *)nullptr, (unsigned long long *)out_keys, out_acc, out_stamps, op, out_capacity,
                           counters, state);
        PCACC_CHECK_LAUNCH();
        return PCACC_OK;
    }
    if (accn_rows_launch(in_acc, in_capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    const int grid = pcacc_grid(m, ACCD_BLOCK);
    hipLaunchKernelGGL(accs_flag_kernel, dim3(grid), dim3(ACCD_BLOCK), 0, st, (const int *)w.rows.dst, m, (const int64_t *)w.kept, mask, mask_rows,
                       invert != 0 ? 1 : 0, w.flag);
    pcacc_scan_i32(w.flag, m, w.chunk, w.spos, st);                                               // spos[m] = rows selected
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accs_move_kernel, dim3(grid), dim3(ACCD_BLOCK), 0, st, keys, in_acc, in_stamps, in_pierced, in_capacity, m, (const int64_t *)w.kept,
                       mask_rows, (const int *)w.flag, (const int *)w.spos, (unsigned long long *)out_keys, out_acc, out_stamps, op, out_capacity, counters,
                       state);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
