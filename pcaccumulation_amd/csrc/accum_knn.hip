// C16. The k nearest kept centroids of the accumulated scene cloud within a few voxels (include/pcacc.h C16).
//
// The map of accum.hip is a sorted key list: the (2r+1)^3 voxels around a query are (2r+1)^2 columns, each a search followed by a walk over at most 2r+1
// consecutive rows, as the normals of C5 and the nearest search of C9 run them, and no other index.  The 2r+1 columns of one x ascend in the list: the
// first is accn_column's search of the whole list, each further one starts at the end of the last run (acck_next_column: doubling steps, then a binary
// search of the last step) -- the same rows, 0.69 of the time at r = 4 (profiles/accum_knn_bench.txt, the interleaved A/B).
//   rows     pass 1 of C5 (accn_rows_launch): dst[m], extract's row of every map row, -1 = filtered out, rows[kept] its inverse; the kept count stays
//            on the device.
//   query    one lane per query in a grid-stride loop, consecutive lanes on consecutive scan points (scan mode) or consecutive kept rows (self mode:
//            their searches land next to each other): acck_point / acck_row of accum_knn.h -- the code the host build runs with every index
//            assert-checked -- then acck_store: every output row written once by the lane of its query.
//   top-k    AcckTop<K> with K = k rounded up to 1, 2, 4, 8 or 16 is a template parameter of the kernel: K slots of (d2, row) that only unrolled loops
//            index, so they stay in registers (profiles/accum_knn_resource_usage.txt: no scratch for any K).
//   counts   the five counts are summed per lane, reduced over the wave, one integer atomic per wave and non-zero counter.
// No floating-point atomics, no LDS beyond the scan's, no inline assembly.  Every result is an integer or a float64 computed in one order, and the
// (d2, row) order of the result is total: two runs give the same bits.
#include "scan.h"
#include "accum_knn.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCK_BLOCK 256
#define ACCK_MAX_POINTS ((int64_t)1 << 30)

static_assert(ACCK_MAX_K == PCACC_KNN_MAX_K && ACCK_MAX_RADIUS == PCACC_KNN_MAX_RADIUS && ACCK_INVALID == PCACC_KNN_INVALID &&
              ACCK_FOUND == PCACC_KNN_FOUND && ACCK_FULL == PCACC_KNN_FULL && ACCK_COUNTERS == PCACC_KNN_COUNTERS &&
              ACCK_C_QUERIES == PCACC_KNN_N_QUERIES && ACCK_C_INVALID == PCACC_KNN_N_INVALID && ACCK_C_FOUND == PCACC_KNN_N_FOUND &&
              ACCK_C_FULL == PCACC_KNN_N_FULL && ACCK_C_NEIGHBORS == PCACC_KNN_N_NEIGHBORS,
              "accum_knn.h and include/pcacc.h name the same limits, bits and counters");

struct AcckCounts { long long queries, invalid, found, full, neighbors; };

static __device__ __forceinline__ void acck_count(AcckCounts &c, int status, int found, int k)
{
    c.queries += 1;
    c.invalid += (status & ACCK_INVALID) != 0;
    c.found += found > 0;
    c.full += found == k;
    c.neighbors += found > 0 ? found : 0;
}

// every lane of the wave arrives here: one atomic per wave and non-zero counter
static __device__ __forceinline__ void acck_counters(unsigned long long *counters, const AcckCounts &c)
{
    accum_wave_count(counters, ACCK_C_QUERIES, c.queries);
    accum_wave_count(counters, ACCK_C_INVALID, c.invalid);
    accum_wave_count(counters, ACCK_C_FOUND, c.found);
    accum_wave_count(counters, ACCK_C_FULL, c.full);
    accum_wave_count(counters, ACCK_C_NEIGHBORS, c.neighbors);
}

template <int K>
static __global__ __launch_bounds__(ACCK_BLOCK) void acck_point_kernel(const float *__restrict__ points, int64_t n, const double *__restrict__ pose,
                                                                        AcckParams P, AcckOut out, unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    double T[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) T[a] = pose ? pose[a] : ((a % 5 == 0) ? 1.0 : 0.0);
    AcckCounts c = {0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * ACCK_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCK_BLOCK) {
        AcckTop<K> top;
        const int status = acck_point(P, T, points + 3 * i, top);
        const int found = acck_store(out, i, n, P.k, top, status);
        acck_count(c, status, found, P.k);
    }
    acck_counters(counters, c);
}

template <int K>
static __global__ __launch_bounds__(ACCK_BLOCK) void acck_self_kernel(AcckParams P, const int *__restrict__ rows, const int64_t *__restrict__ kept_ptr,
                                                                       AcckOut out, unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    int64_t kept = *kept_ptr;
    if (kept > P.m) kept = P.m;                                                              // every output has room for m rows
    AcckCounts c = {0, 0, 0, 0, 0};
    for (int64_t j = (int64_t)blockIdx.x * ACCK_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCK_BLOCK) {
        const int64_t i = rows[j];
        AcckTop<K> top;
        if (i < 0 || i >= P.m || P.dst[i] != j) continue;                                    // a table that does not fit addresses nothing
        if (!acck_row(P, i, top)) continue;
        const int found = acck_store(out, j, kept, P.k, top, 0);
        acck_count(c, 0, found, P.k);
    }
    acck_counters(counters, c);
}

template <int K>
static void acck_launch(const float *points, int64_t n, const double *pose, const AcckParams &P, const int *rows, const int64_t *kept, const AcckOut &out,
                        int64_t *counters, hipStream_t st)
{
    // a lane runs (2r+1)^2 serial searches: many small workgroups spread over the CUs, as accum_normals.hip
    if (points)
        hipLaunchKernelGGL(acck_point_kernel<K>, dim3(pcacc_grid(n, ACCK_BLOCK, 1 << 22)), dim3(ACCK_BLOCK), 0, st, points, n, pose, P, out,
                           (unsigned long long *)counters);
    else
        hipLaunchKernelGGL(acck_self_kernel<K>, dim3(pcacc_grid(P.m, ACCK_BLOCK, 1 << 22)), dim3(ACCK_BLOCK), 0, st, P, rows, kept, out,
                           (unsigned long long *)counters);
}

// points != NULL: scan mode over n points; else self mode over the kept rows.
static int acck_dispatch(const float *points, int64_t n, const double *pose, const AcckParams &P, const int *rows, const int64_t *kept, const AcckOut &out,
                         int64_t *counters, hipStream_t st)
{
    switch (acck_slots(P.k)) {
    case 1: acck_launch<1>(points, n, pose, P, rows, kept, out, counters, st); break;
    case 2: acck_launch<2>(points, n, pose, P, rows, kept, out, counters, st); break;
    case 4: acck_launch<4>(points, n, pose, P, rows, kept, out, counters, st); break;
    case 8: acck_launch<8>(points, n, pose, P, rows, kept, out, counters, st); break;
    case 16: acck_launch<16>(points, n, pose, P, rows, kept, out, counters, st); break;
    default: return PCACC_E_ARG;
    }
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// What both entry points check of the map and the search.
static bool acck_bad_args(double voxel_size, double max_distance, int32_t k, int32_t radius, const int64_t *keys, const int64_t *acc, int64_t capacity,
                          int64_t m, const int64_t *counters, const void *workspace)
{
    if (k < 1 || k > ACCK_MAX_K || radius < 1 || radius > ACCK_MAX_RADIUS) return true;
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY) return true;
    if (!(voxel_size > 0.0) || !(voxel_size < 1e300) || !(max_distance > 0.0) || !(max_distance <= (double)radius * voxel_size)) return true;
    return !counters || !workspace || (m > 0 && (!keys || !acc));
}

extern "C" int pcacc_accum_knn_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccnRowsWs w;
    *bytes = accn_rows_ws_carve(m, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_knn(const float *points, int64_t n, const double *pose, double voxel_size, double max_distance, int32_t k, int32_t radius,
                               const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                               double max_moving_fraction, int32_t *out_rows, double *out_distance, int32_t *out_found, uint8_t *out_status,
                               int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > ACCK_MAX_POINTS || acck_bad_args(voxel_size, max_distance, k, radius, keys, acc, capacity, m, counters, workspace)) return PCACC_E_ARG;
    if (n > 0 && (!points || !out_rows || !out_distance || !out_found || !out_status)) return PCACC_E_ARG;
    AccnRowsWs w;
    if (workspace_bytes < accn_rows_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCK_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (n == 0) return PCACC_OK;
    if (m > 0 && accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    AcckParams P;
    P.keys = (const unsigned long long *)keys; P.acc = acc; P.dst = w.rows.dst;
    P.capacity = capacity; P.m = m; P.voxel_size = voxel_size; P.max_d2 = max_distance * max_distance; P.radius = radius; P.k = k;
    const AcckOut out = {out_rows, out_distance, out_found, out_status, nullptr};
    return acck_dispatch(points, n, pose, P, nullptr, nullptr, out, counters, st);
}

extern "C" int pcacc_accum_knn_self(double voxel_size, double max_distance, int32_t k, int32_t radius, const int64_t *keys, const int64_t *acc,
                                    int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction,
                                    int32_t *out_rows, double *out_distance, int32_t *out_found, uint8_t *out_status, double *out_mean_distance,
                                    int64_t *out_n, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!out_n || acck_bad_args(voxel_size, max_distance, k, radius, keys, acc, capacity, m, counters, workspace)) return PCACC_E_ARG;
    if (m > 0 && (!out_rows || !out_distance || !out_found || !out_status || !out_mean_distance)) return PCACC_E_ARG;
    AccnRowsWs w;
    if (workspace_bytes < accn_rows_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCK_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return hipMemsetAsync(out_n, 0, sizeof(int64_t), st) == hipSuccess ? PCACC_OK : PCACC_E_LAUNCH;
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    if (hipMemcpyAsync(out_n, w.kept, sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return PCACC_E_LAUNCH;
    AcckParams P;
    P.keys = (const unsigned long long *)keys; P.acc = acc; P.dst = w.rows.dst;
    P.capacity = capacity; P.m = m; P.voxel_size = voxel_size; P.max_d2 = max_distance * max_distance; P.radius = radius; P.k = k;
    const AcckOut out = {out_rows, out_distance, out_found, out_status, out_mean_distance};
    return acck_dispatch(nullptr, 0, nullptr, P, (const int *)w.rows.rows, (const int64_t *)w.kept, out, counters, st);
}
