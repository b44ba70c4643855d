// C7. Rays through the accumulated scene cloud: how many measured rays pass through each voxel of the map (include/pcacc.h C7).
//
// One lane per ray; the whole of a ray is accp_ray of accum_pierce.h -- the code the host build runs with every index assert-checked.  Consecutive points
// of a scan are neighbouring beams: the lanes of a wave walk through the same part of the sorted key list.  The only writes are integer atomics: one per
// counted visit on pierced[row], and one per wave and counter after a reduction over the 64 lanes.  No floating-point atomics, no LDS, no inline assembly.
#include "common.h"
#include "accum_pierce.h"
#include "accum_launch.h"

#define ACCP_BLOCK 256
#define ACCP_MAX_POINTS ((int64_t)1 << 30)

struct AccpHit {
    int32_t *pierced;
    __device__ __forceinline__ void operator()(int64_t pos) const { atomicAdd(&pierced[pos], 1); }
};

static __global__ __launch_bounds__(ACCP_BLOCK) void accp_pierce_kernel(const float *__restrict__ points, int64_t n, const uint8_t *__restrict__ moving,
                                                                         const double *__restrict__ origins, int64_t n_origins,
                                                                         const int32_t *__restrict__ origin_index, const double *__restrict__ pose,
                                                                         double voxel_size, double margin, int use_range, double max_range, int use_stamp,
                                                                         int32_t stamp, int max_steps, const unsigned long long *__restrict__ keys,
                                                                         const int32_t *__restrict__ stamps, int64_t capacity, int64_t m,
                                                                         int32_t *__restrict__ pierced, unsigned long long *__restrict__ counters)
{
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);        // NULL = identity, through the same arithmetic
    AccpHit hit = {pierced};
    long long c_walked = 0, c_dropped = 0, c_skipped = 0, c_truncated = 0, c_hits = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCP_BLOCK) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        const int64_t row = accp_origin_index(origin_index ? (int64_t)origin_index[i] : 0, n_origins);
        double o[3] = {0.0, 0.0, 0.0};
        if (row >= 0) { o[0] = origins[3 * row]; o[1] = origins[3 * row + 1]; o[2] = origins[3 * row + 2]; }
        const AccpRay r = accp_ray(T, p, o, row >= 0, moving && moving[i], voxel_size, margin, use_range != 0, max_range,
                                             use_stamp != 0, stamp, max_steps, keys, stamps, capacity, m, hit);
        c_walked += r.status == ACCP_WALKED; c_dropped += r.status == ACCP_DROPPED; c_skipped += r.status == ACCP_SKIPPED;
        c_truncated += r.truncated; c_hits += r.hits;
    }
    // every lane of the wave arrives here: one atomic per wave and counter
    accum_wave_count(counters, PCACC_PIERCE_WALKED, c_walked);
    accum_wave_count(counters, PCACC_PIERCE_DROPPED, c_dropped);
    accum_wave_count(counters, PCACC_PIERCE_SKIPPED, c_skipped);
    accum_wave_count(counters, PCACC_PIERCE_TRUNCATED, c_truncated);
    accum_wave_count(counters, PCACC_PIERCE_HITS, c_hits);
}

// No launch of C7 takes scratch memory today; the pair of entry points keeps the calling convention of C4 - C6.
extern "C" int pcacc_accum_pierce_workspace_bytes(int64_t n, int64_t m, size_t *bytes)
{
    if (!bytes || n < 0 || n > ACCP_MAX_POINTS || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    *bytes = 0;
    return PCACC_OK;
}

extern "C" int pcacc_accum_pierce(const float *points, int64_t n, const uint8_t *moving, const double *origins, int64_t n_origins,
                                  const int32_t *origin_index, const double *pose, double voxel_size, double margin, double max_range,
                                  int32_t use_stamp, int32_t stamp, int32_t max_steps, const int64_t *keys, const int32_t *stamps, int64_t capacity,
                                  int64_t m, int32_t *pierced, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (n < 0 || n > ACCP_MAX_POINTS || n_origins < 1 || m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    if (!(margin >= 0.0) || !(margin - margin == 0.0) || max_range != max_range) return PCACC_E_ARG;
    if (max_steps < 1 || max_steps > ACCP_MAX_STEPS || !counters) return PCACC_E_ARG;
    if (n == 0) return PCACC_OK;
    if (!points || !origins) return PCACC_E_ARG;
    if (m > 0 && (!keys || !stamps || !pierced)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    // a lane walks hundreds of voxels with a search each: many small workgroups spread over the CUs, as accum_normals.hip
    const dim3 grid(pcacc_grid(n, ACCP_BLOCK, 1 << 22)), block(ACCP_BLOCK);
    const int use_range = max_range >= 0.0 ? 1 : 0;
    // m = 0: the rays are classified and walked, the search answers 0 without a load and no table is addressed
    hipLaunchKernelGGL(accp_pierce_kernel, grid, block, 0, st, points, n, moving, origins, n_origins, origin_index, pose, voxel_size, margin, use_range, max_range,
                       (int)use_stamp, stamp, (int)max_steps, (const unsigned long long *)keys, stamps, capacity, m, pierced, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
