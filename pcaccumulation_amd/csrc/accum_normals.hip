// C5. Per-voxel surface normals of the accumulated scene cloud (include/pcacc.h C5).
//
// The map of accum.hip is a sorted, duplicate-free key list whose low bits are z: the neighbourhood of a voxel is (2r+1)^2 binary searches, each
// followed by a walk over at most 2r+1 consecutive rows.  No hash table, no floating-point atomics, no LDS beyond the scan's, no inline assembly.
//   pass 1   keep flags (extract's predicate) -> scan.h -> dst[m]: output row of every map row, -1 = does not participate; rows[kept]: its inverse.
//            (accn_rows_launch of accum_rows.h: accum_register.hip calls the same launch sequence.)  dst serves as the neighbour test AND the output row: a neighbour costs one gather, not a re-evaluation of the predicate.
//   pass 2   one lane per participating row, consecutive lanes on consecutive rows (their searches land next to each other); the whole result of a
//            voxel is accum_normal_voxel of accum_normals.h -- the code the host build runs with every index assert-checked; outputs written once.
// Everything a result depends on is the set of integer records, visited in key order: two runs give the same bits.
#include "scan.h"
#include "accum_normals.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCN_BLOCK 256
static_assert(ACCN_BLOCK == ACCUM_KEEP_BLOCK, "accn_rows_launch launches accum_keep_kernel on the grid of accn_dst_kernel");

// keep[i] (0 / 1) becomes dst[i] in place; rows[dst[i]] = i.
static __global__ __launch_bounds__(ACCN_BLOCK) void accn_dst_kernel(int *__restrict__ keep_dst, const int *__restrict__ kpos, int64_t m, int *__restrict__ rows,
                                                                      int64_t *out_n)
{
    const int64_t kept = kpos[m];
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_n = kept;
    for (int64_t i = (int64_t)blockIdx.x * ACCN_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCN_BLOCK) {
        const int64_t d = keep_dst[i] ? accum_merge_dst(kpos[i], 0, kept) : -1;              // in [0, kept), kept <= m = entries of rows
        keep_dst[i] = (int)d;
        if (d >= 0) rows[d] = (int)i;
    }
}

static __global__ __launch_bounds__(ACCN_BLOCK) void accn_normals_kernel(const unsigned long long *__restrict__ keys, const int64_t *__restrict__ acc,
                                                                          const int32_t *__restrict__ stamps, int64_t capacity, int64_t m,
                                                                          const int *__restrict__ dst, const int *__restrict__ rows,
                                                                          const int *__restrict__ kept_ptr, int radius, int min_neighbors,
                                                                          const double *__restrict__ viewpoints, int64_t n_viewpoints, int64_t stamp_base,
                                                                          float *__restrict__ out_normals, float *__restrict__ out_eigenvalues,
                                                                          int32_t *__restrict__ out_neighbors, uint8_t *__restrict__ out_flags)
{
    int64_t kept = *kept_ptr;
    if (kept > m) kept = m;                                                                  // every output has room for m rows
    for (int64_t j = (int64_t)blockIdx.x * ACCN_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCN_BLOCK) {
        const int64_t i = rows[j];
        AccnResult r;
        if (i < 0 || i >= m || dst[i] != j) continue;                                        // a table that does not fit addresses nothing
        if (!accum_normal_voxel(keys, acc, stamps, capacity, m, dst, i, radius, min_neighbors, viewpoints, n_viewpoints, stamp_base, &r)) continue;
        out_normals[3 * j] = (float)r.normal[0]; out_normals[3 * j + 1] = (float)r.normal[1]; out_normals[3 * j + 2] = (float)r.normal[2];
        out_eigenvalues[3 * j] = (float)r.s[0]; out_eigenvalues[3 * j + 1] = (float)r.s[1]; out_eigenvalues[3 * j + 2] = (float)r.s[2];
        out_neighbors[j] = r.k;
        out_flags[j] = (uint8_t)r.flags;
    }
}

size_t accn_rows_carve(int64_t m, AccnRows *t, char *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    t->dst = (int *)take((size_t)m * 4);
    t->kpos = (int *)take((size_t)(m + 1) * 4);
    t->rows = (int *)take((size_t)m * 4);
    t->chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    return off;
}

int accn_rows_launch(const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int use_fraction, double max_moving_fraction, const AccnRows &t,
                     int64_t *out_n, hipStream_t st)
{
    const int grid = pcacc_grid(m, ACCN_BLOCK);
    hipLaunchKernelGGL(accum_keep_kernel, dim3(grid), dim3(ACCN_BLOCK), 0, st, acc, capacity, m, min_count, use_fraction, max_moving_fraction, t.dst);
    pcacc_scan_i32(t.dst, m, t.chunk, t.kpos, st);                                           // kpos[m] = kept
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accn_dst_kernel, dim3(grid), dim3(ACCN_BLOCK), 0, st, t.dst, (const int *)t.kpos, m, t.rows, out_n);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

extern "C" int pcacc_accum_normals_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccnRows t;
    *bytes = accn_rows_carve(m > 0 ? m : 1, &t, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_normals(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                                   int32_t use_fraction, double max_moving_fraction, int32_t radius, int32_t min_neighbors, const double *viewpoints,
                                   int64_t n_viewpoints, int64_t stamp_base, float *out_normals, float *out_eigenvalues, int32_t *out_neighbors,
                                   uint8_t *out_flags, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || !out_n) return PCACC_E_ARG;
    if (radius < 1 || radius > ACCN_MAX_RADIUS || min_neighbors < ACCN_MIN_NEIGHBORS || n_viewpoints < 0) return PCACC_E_ARG;
    if (n_viewpoints > 0 && !viewpoints) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (m == 0) return hipMemsetAsync(out_n, 0, sizeof(int64_t), st) == hipSuccess ? PCACC_OK : PCACC_E_LAUNCH;
    if (!keys || !acc || !stamps || !out_normals || !out_eigenvalues || !out_neighbors || !out_flags || !workspace) return PCACC_E_ARG;
    AccnRows t;
    if (workspace_bytes < accn_rows_carve(m, &t, (char *)workspace)) return PCACC_E_WORKSPACE;
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, t, out_n, st) != PCACC_OK) return PCACC_E_LAUNCH;
    const int *dst = t.dst, *rows = t.rows, *kpos = t.kpos;
    // a lane carries ~100 VGPRs of float64 state and serial searches: many small workgroups spread over the CUs, not a short grid-stride loop
    hipLaunchKernelGGL(accn_normals_kernel, dim3(pcacc_grid(m, ACCN_BLOCK, 1 << 22)), dim3(ACCN_BLOCK), 0, st, (const unsigned long long *)keys, acc, stamps,
                       capacity, m, (const int *)dst, (const int *)rows, (const int *)(kpos + m), (int)radius, (int)min_neighbors,
                       n_viewpoints > 0 ? viewpoints : (const double *)nullptr, n_viewpoints, stamp_base, out_normals, out_eigenvalues, out_neighbors, out_flags);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
