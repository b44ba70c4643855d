// C9. Looking a scan's points up in the accumulated scene cloud (include/pcacc.h C9).
//
// The map of accum.hip is a sorted key list: a scan point finds its own voxel with one binary search and its nearest kept centroid with the nine column
// searches of accr_match (accn_column, r = 1), as a registration round does, and no other index.
//   rows     pass 1 of C5 (accn_rows_launch): dst[m], extract's row of every map row, -1 = filtered out; the kept count stays on the device.
//   point    one lane per scan point in a grid-stride loop, consecutive lanes on consecutive points: accq_point of accum_query.h -- the code the host
//            build runs with every index assert-checked -- then accq_store: every output column as the coalesced column it is, every row written once
//            by the lane of its point.  The six counts are summed per lane, reduced over the wave, one integer atomic per wave and non-zero counter.
// The kernel compares the kept count with n_rows itself (BAD_TABLE): nothing is read back.  No floating-point atomics, no LDS beyond the scan's, no
// inline assembly.  Every result is an integer, a copied record or a float64 computed in one order: two runs give the same bits.
#include "scan.h"
#include "accum_query.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCQ_BLOCK 256
#define ACCQ_MAX_POINTS ((int64_t)1 << 30)

static_assert(ACCQ_INVALID == PCACC_QUERY_INVALID && ACCQ_OCCUPIED == PCACC_QUERY_OCCUPIED && ACCQ_KEPT == PCACC_QUERY_KEPT &&
              ACCQ_MATCHED == PCACC_QUERY_MATCHED && ACCQ_NORMAL == PCACC_QUERY_NORMAL && ACCQ_COUNTERS == PCACC_QUERY_COUNTERS &&
              ACCQ_C_POINTS == PCACC_QUERY_N_POINTS && ACCQ_C_NORMAL == PCACC_QUERY_N_NORMAL && ACCQ_C_BAD_TABLE == PCACC_QUERY_BAD_TABLE,
              "accum_query.h and include/pcacc.h name the same bits and counters");

static __global__ __launch_bounds__(ACCQ_BLOCK) void accq_point_kernel(const float *__restrict__ points, int64_t n, const double *__restrict__ pose,
                                                                        AccqParams P, const int64_t *__restrict__ kept_ptr, AccqOut out,
                                                                        unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    const int tables = accq_tables(P.normals != nullptr, kept_ptr ? *kept_ptr : 0, P.n_rows);         // uniform over the grid
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    long long c_points = 0, c_invalid = 0, c_occupied = 0, c_kept = 0, c_matched = 0, c_normal = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCQ_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCQ_BLOCK) {
        AccqRecord r;
        accq_point(P, tables, T, points + 3 * i, &r);
        accq_store(out, i, n, r);
        c_points += 1;
        c_invalid += (r.status & ACCQ_INVALID) != 0; c_occupied += (r.status & ACCQ_OCCUPIED) != 0; c_kept += (r.status & ACCQ_KEPT) != 0;
        c_matched += (r.status & ACCQ_MATCHED) != 0; c_normal += (r.status & ACCQ_NORMAL) != 0;
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACCQ_C_POINTS, c_points);
    accum_wave_count(counters, ACCQ_C_INVALID, c_invalid);
    accum_wave_count(counters, ACCQ_C_OCCUPIED, c_occupied);
    accum_wave_count(counters, ACCQ_C_KEPT, c_kept);
    accum_wave_count(counters, ACCQ_C_MATCHED, c_matched);
    accum_wave_count(counters, ACCQ_C_NORMAL, c_normal);
    if (blockIdx.x == 0 && threadIdx.x == 0 && tables == ACCQ_BAD_TABLES) counters[ACCQ_C_BAD_TABLE] = 1;   // the memset left 0; no lane adds to this one
}

extern "C" int pcacc_accum_query_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccnRowsWs w;
    *bytes = accn_rows_ws_carve(m, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_query(const float *points, int64_t n, const double *pose, double voxel_size, double max_distance, const int64_t *keys,
                                 const int64_t *acc, const int32_t *stamps, const int32_t *pierced, int64_t capacity, int64_t m, int64_t min_count,
                                 int32_t use_fraction, double max_moving_fraction, const float *normals, const uint8_t *flags, int64_t n_rows,
                                 int32_t require_normal, uint8_t *out_status, int64_t *out_count, int64_t *out_moving, int32_t *out_t_first,
                                 int32_t *out_t_last, int32_t *out_pierced, int32_t *out_row, float *out_nearest, double *out_distance,
                                 double *out_plane_distance, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > ACCQ_MAX_POINTS || m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || n_rows < 0 || n_rows > m) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size < 1e300) || !(max_distance > 0.0) || !(max_distance <= voxel_size)) return PCACC_E_ARG;
    if ((normals != nullptr) != (flags != nullptr) || (require_normal && !normals) || (n_rows > 0 && !normals)) return PCACC_E_ARG;
    if (!counters || !workspace || (m > 0 && (!keys || !acc || !stamps))) return PCACC_E_ARG;
    if (n > 0 && (!points || !out_status || !out_count || !out_moving || !out_t_first || !out_t_last || !out_pierced || !out_row || !out_nearest ||
                  !out_distance || !out_plane_distance))
        return PCACC_E_ARG;
    AccnRowsWs w;
    if (workspace_bytes < accn_rows_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCQ_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (n == 0) return PCACC_OK;
    if (m > 0 && accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    AccqParams P;
    P.keys = (const unsigned long long *)keys; P.acc = acc; P.stamps = stamps; P.pierced = pierced; P.dst = w.rows.dst; P.normals = normals; P.flags = flags;
    P.capacity = capacity; P.m = m; P.n_rows = n_rows; P.min_count = min_count;
    P.voxel_size = voxel_size; P.max_d2 = max_distance * max_distance; P.max_moving_fraction = max_moving_fraction;
    P.use_fraction = use_fraction != 0; P.require_normal = require_normal != 0;
    const AccqOut out = {out_status, out_count, out_moving, out_t_first, out_t_last, out_pierced, out_row, out_nearest, out_distance, out_plane_distance};
    // a lane runs ten serial searches: many small workgroups spread over the CUs, as accum_normals.hip
    hipLaunchKernelGGL(accq_point_kernel, dim3(pcacc_grid(n, ACCQ_BLOCK, 1 << 22)), dim3(ACCQ_BLOCK), 0, st, points, n, pose, P,
                       m > 0 ? (const int64_t *)w.kept : (const int64_t *)nullptr, out, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
