// C10. Casting rays into the accumulated scene cloud: per ray the first voxel the map keeps and its range (include/pcacc.h C10).
//
//   rows     pass 1 of C5 (accn_rows_launch): dst[m], extract's row of every map row, -1 = filtered out, as C9 gets it.
//   ray      one lane per ray in a grid-stride loop, consecutive lanes on consecutive rays (neighbouring beams walk through the same part of the sorted
//            key list): accy_ray of accum_raycast.h -- the code the host build runs with every index assert-checked -- then accy_store: every output
//            column as the coalesced column it is, every row written once by the lane of its ray.  The map is only read.
// The rays of a wave end at different visits; the contract fixes the result, not the route, and nothing is compacted or queued again.  The seven counts
// are summed per lane, reduced over the wave, one integer atomic per wave and non-zero counter.  No floating-point atomics, no LDS beyond the scan's, no
// inline assembly.  Every result is an integer, a copied value or a float64 computed in one order: two runs give the same bits.
#include "scan.h"
#include "accum_raycast.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCY_BLOCK 256
#define ACCY_MAX_RAYS ((int64_t)1 << 30)

static_assert(ACCY_MISS == PCACC_RAYCAST_MISS && ACCY_HIT == PCACC_RAYCAST_HIT && ACCY_TRUNCATED == PCACC_RAYCAST_TRUNCATED &&
              ACCY_SKIPPED == PCACC_RAYCAST_SKIPPED && ACCY_DROPPED == PCACC_RAYCAST_DROPPED && ACCY_COUNTERS == PCACC_RAYCAST_COUNTERS &&
              ACCY_C_RAYS == PCACC_RAYCAST_N_RAYS && ACCY_C_DROPPED == PCACC_RAYCAST_N_DROPPED && ACCY_C_SKIPPED == PCACC_RAYCAST_N_SKIPPED &&
              ACCY_C_HIT == PCACC_RAYCAST_N_HIT && ACCY_C_MISSED == PCACC_RAYCAST_N_MISSED && ACCY_C_TRUNCATED == PCACC_RAYCAST_N_TRUNCATED &&
              ACCY_C_VISITS == PCACC_RAYCAST_N_VISITS,
              "accum_raycast.h and include/pcacc.h name the same codes and counters");

static __global__ __launch_bounds__(ACCY_BLOCK) void accy_ray_kernel(const float *__restrict__ targets, int64_t n, const double *__restrict__ origins,
                                                                      int64_t n_origins, const int32_t *__restrict__ origin_index,
                                                                      const double *__restrict__ pose, AccyParams P, AccyOut out,
                                                                      unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);        // NULL = identity, through the same arithmetic
    long long c_rays = 0, c_dropped = 0, c_skipped = 0, c_hit = 0, c_missed = 0, c_truncated = 0, c_visits = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCY_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCY_BLOCK) {
        const float p[3] = {targets[3 * i], targets[3 * i + 1], targets[3 * i + 2]};
        const int64_t row = accp_origin_index(origin_index ? (int64_t)origin_index[i] : 0, n_origins);
        double o[3] = {0.0, 0.0, 0.0};
        if (row >= 0) { o[0] = origins[3 * row]; o[1] = origins[3 * row + 1]; o[2] = origins[3 * row + 2]; }
        AccyRecord r;
        accy_ray(P, T, p, o, row >= 0, &r);
        accy_store(out, i, n, r);
        c_rays += 1;
        c_dropped += r.status == ACCY_DROPPED; c_skipped += r.status == ACCY_SKIPPED; c_hit += r.status == ACCY_HIT;
        c_missed += r.status == ACCY_MISS; c_truncated += r.status == ACCY_TRUNCATED; c_visits += r.visits;
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACCY_C_RAYS, c_rays);
    accum_wave_count(counters, ACCY_C_DROPPED, c_dropped);
    accum_wave_count(counters, ACCY_C_SKIPPED, c_skipped);
    accum_wave_count(counters, ACCY_C_HIT, c_hit);
    accum_wave_count(counters, ACCY_C_MISSED, c_missed);
    accum_wave_count(counters, ACCY_C_TRUNCATED, c_truncated);
    accum_wave_count(counters, ACCY_C_VISITS, c_visits);
}

extern "C" int pcacc_accum_raycast_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccnRowsWs w;
    *bytes = accn_rows_ws_carve(m, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_raycast(const float *targets, int64_t n, const double *origins, int64_t n_origins, const int32_t *origin_index,
                                   const double *pose, double voxel_size, double min_range, double max_range, double margin, int32_t max_steps,
                                   const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                                   double max_moving_fraction, uint8_t *out_status, int32_t *out_row, int32_t *out_coords, float *out_point,
                                   double *out_range_in, double *out_depth, double *out_length, int32_t *out_visits, int64_t *counters, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > ACCY_MAX_RAYS || n_origins < 1 || m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    if (!(min_range >= 0.0) || !(min_range - min_range == 0.0) || !(margin >= 0.0) || !(margin - margin == 0.0) || max_range != max_range) return PCACC_E_ARG;
    if (max_steps < 1 || max_steps > ACCY_MAX_STEPS) return PCACC_E_ARG;
    if (!counters || !workspace || (m > 0 && (!keys || !acc))) return PCACC_E_ARG;
    if (n > 0 && (!targets || !origins || !out_status || !out_row || !out_coords || !out_point || !out_range_in || !out_depth || !out_length || !out_visits))
        return PCACC_E_ARG;
    AccnRowsWs w;
    if (workspace_bytes < accn_rows_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCY_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (n == 0) return PCACC_OK;
    if (m > 0 && accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    AccyParams P;
    P.keys = (const unsigned long long *)keys; P.acc = acc; P.dst = w.rows.dst;
    P.capacity = capacity; P.m = m;
    P.voxel_size = voxel_size; P.min_range = min_range; P.margin = margin; P.max_range = max_range;
    P.use_range = max_range >= 0.0 ? 1 : 0; P.max_steps = (int)max_steps;
    const AccyOut out = {out_status, out_row, out_coords, out_point, out_range_in, out_depth, out_length, out_visits};
    // a lane walks up to hundreds of voxels with a search each: many small workgroups spread over the CUs, as accum_pierce.hip
    // m = 0: the rays are classified and walked, the search answers 0 without a load and no table is addressed
    hipLaunchKernelGGL(accy_ray_kernel, dim3(pcacc_grid(n, ACCY_BLOCK, 1 << 22)), dim3(ACCY_BLOCK), 0, st, targets, n, origins, n_origins, origin_index, pose, P,
                       out, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
