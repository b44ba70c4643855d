// C8. Removing rows from the accumulated scene cloud: pierced, stale, far and isolated voxels leave the map on the device (include/pcacc.h C8,
// DESIGN.md section 9g).
//
//   stage A   one lane per map row: the reason the row leaves (accr_row_reason of accum_prune.h, from the row's record alone) -> keep flag, reason
//   scan      scan.h over the flags -> kpos; with stage B: dst[m] (output row or -1, the neighbour test) and rows[survivors], its inverse
//   stage B   one lane per stage-A survivor, consecutive lanes on consecutive rows: (2r+1)^2 column searches (accr_neighbors), flag and reason
//             updated; a second scan.  dst is not touched: k counts stage-A survivors whatever stage B decides next door.
//   compact   survivor i -> row accum_merge_dst(kpos[i], 0, kept) of the output tables, every column as the coalesced column it is, every destination
//             written once; the six counters summed per lane, reduced over the wave, one integer atomic per wave and non-zero counter; one thread
//             writes the state word.
// The functions are those the host build runs with every index assert-checked.  No floating-point atomics, no LDS beyond the scan's, no inline
// assembly; nothing is read back.
#include "scan.h"
#include "accum_prune.h"
#include "accum_launch.h"

#define ACCR_BLOCK 256

static __global__ __launch_bounds__(ACCR_BLOCK) void accr_reason_kernel(const unsigned long long *__restrict__ keys, const int64_t *__restrict__ acc,
                                                                         const int32_t *__restrict__ stamps, const int32_t *__restrict__ pierced,
                                                                         int64_t capacity, int64_t m, AccrParams P, int *__restrict__ flag,
                                                                         uint8_t *__restrict__ reason)
{
    for (int64_t i = (int64_t)blockIdx.x * ACCR_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCR_BLOCK) {
        const int r = accr_row_reason(keys, acc, stamps, pierced, capacity, m, i, P);
        flag[i] = r == ACCR_KEPT ? 1 : 0;
        reason[i] = (uint8_t)r;
    }
}

// dst[i] = output row of stage-A survivor i, -1 otherwise; rows[dst[i]] = i.
static __global__ __launch_bounds__(ACCR_BLOCK) void accr_dst_kernel(const int *__restrict__ flag, const int *__restrict__ kpos, int64_t m, int *__restrict__ dst,
                                                                      int *__restrict__ rows)
{
    const int64_t kept = kpos[m];
    for (int64_t i = (int64_t)blockIdx.x * ACCR_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCR_BLOCK) {
        const int64_t d = flag[i] ? accum_merge_dst(kpos[i], 0, kept) : -1;                  // in [0, kept), kept <= m = entries of rows
        dst[i] = (int)d;
        if (d >= 0) rows[d] = (int)i;
    }
}

static __global__ __launch_bounds__(ACCR_BLOCK) void accr_isolated_kernel(const unsigned long long *__restrict__ keys, int64_t m, const int *__restrict__ dst,
                                                                           const int *__restrict__ rows, const int *__restrict__ kept_ptr, int radius,
                                                                           int min_neighbors, int *__restrict__ flag, uint8_t *__restrict__ reason)
{
    int64_t kept = *kept_ptr;
    if (kept > m) kept = m;
    for (int64_t j = (int64_t)blockIdx.x * ACCR_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCR_BLOCK) {
        const int64_t i = rows[j];
        if (i < 0 || i >= m || dst[i] != j) continue;                                        // a table that does not fit addresses nothing
        if (accr_neighbors(keys, m, dst, i, radius) < min_neighbors) {
            flag[i] = 0;
            reason[i] = ACCR_ISOLATED;
        }
    }
}

static __global__ __launch_bounds__(ACCR_BLOCK) void accr_compact_kernel(const unsigned long long *__restrict__ in_keys, const int64_t *__restrict__ in_acc,
                                                                          const int32_t *__restrict__ in_stamps, const int32_t *__restrict__ in_pierced,
                                                                          int64_t in_capacity, int64_t m, const int *__restrict__ flag,
                                                                          const int *__restrict__ kpos, const uint8_t *__restrict__ reason, int dry_run,
                                                                          unsigned long long *__restrict__ out_keys, int64_t *__restrict__ out_acc,
                                                                          int32_t *__restrict__ out_stamps, int32_t *__restrict__ out_pierced,
                                                                          int64_t out_capacity, unsigned long long *__restrict__ counters,
                                                                          int64_t *__restrict__ state)
{
    const int64_t kept = kpos[m];
    long long c_kept = 0, c_filter = 0, c_stale = 0, c_box = 0, c_pierced = 0, c_isolated = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCR_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCR_BLOCK) {
        const int r = reason[i];
        c_kept += r == ACCR_KEPT; c_filter += r == ACCR_FILTER; c_stale += r == ACCR_STALE; c_box += r == ACCR_BOX; c_pierced += r == ACCR_PIERCED;
        c_isolated += r == ACCR_ISOLATED;
        if (dry_run || !flag[i]) continue;
        accr_move_row(in_keys, in_acc, in_stamps, in_pierced, in_capacity, m, i, out_keys, out_acc, out_stamps, out_pierced, out_capacity, kept,
                      accum_merge_dst(kpos[i], 0, kept));
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, PCACC_PRUNE_KEPT, c_kept);
    accum_wave_count(counters, PCACC_PRUNE_FILTER, c_filter);
    accum_wave_count(counters, PCACC_PRUNE_STALE, c_stale);
    accum_wave_count(counters, PCACC_PRUNE_BOX, c_box);
    accum_wave_count(counters, PCACC_PRUNE_PIERCED, c_pierced);
    accum_wave_count(counters, PCACC_PRUNE_ISOLATED, c_isolated);
    if (!dry_run && blockIdx.x == 0 && threadIdx.x == 0) state[PCACC_ACCUM_NUM_VOXELS] = kept;
}

struct AccrWs { int *flag, *kpos, *dst, *rows, *chunk; uint8_t *reason; };

static size_t accr_carve(int64_t m, AccrWs *t, char *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    t->flag = (int *)take((size_t)m * 4);
    t->kpos = (int *)take((size_t)(m + 1) * 4);
    t->dst = (int *)take((size_t)m * 4);
    t->rows = (int *)take((size_t)m * 4);
    t->chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    t->reason = (uint8_t *)take((size_t)m);
    return off;
}

extern "C" int pcacc_accum_prune_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccrWs t;
    *bytes = accr_carve(m > 0 ? m : 1, &t, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_prune(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                                 int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction, int32_t use_stamp, int32_t before_stamp,
                                 int32_t use_box, int32_t lo_x, int32_t lo_y, int32_t lo_z, int32_t hi_x, int32_t hi_y, int32_t hi_z, int32_t min_pierced,
                                 int32_t use_ratio, double ratio, int32_t min_neighbors, int32_t radius, int32_t dry_run, int64_t *out_keys,
                                 int64_t *out_acc, int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || in_capacity < m || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < m || out_capacity > ACCUM_MAX_CAPACITY || !counters) return PCACC_E_ARG;
    if (min_neighbors < 0 || min_neighbors > ACCR_MAX_NEIGHBORS) return PCACC_E_ARG;
    if (min_neighbors > 0 && (radius < 1 || radius > ACCN_MAX_RADIUS)) return PCACC_E_ARG;
    if (use_ratio && !(ratio >= 0.0)) return PCACC_E_ARG;                                    // NaN or negative
    if (use_box) {
        const int32_t lo[3] = {lo_x, lo_y, lo_z}, hi[3] = {hi_x, hi_y, hi_z};
        for (int a = 0; a < 3; ++a)
            if (lo[a] > hi[a] || !accn_in_range(lo[a]) || !accn_in_range(hi[a])) return PCACC_E_ARG;
    }
    if (accum_tables_overlap(in_keys, in_acc, in_stamps, in_pierced, in_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    AccrWs t;
    if (m > 0) {
        if (!in_keys || !in_acc || !in_stamps || !workspace) return PCACC_E_ARG;
        if (!dry_run && (!out_keys || !out_acc || !out_stamps || !state || (in_pierced && !out_pierced))) return PCACC_E_ARG;
        if (workspace_bytes < accr_carve(m, &t, (char *)workspace)) return PCACC_E_WORKSPACE;
    }
    if (hipMemsetAsync(counters, 0, ACCR_REASONS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return PCACC_OK;
    AccrParams P;
    P.min_count = min_count; P.max_moving_fraction = max_moving_fraction; P.ratio = ratio; P.before_stamp = before_stamp;
    P.lo_x = lo_x; P.lo_y = lo_y; P.lo_z = lo_z; P.hi_x = hi_x; P.hi_y = hi_y; P.hi_z = hi_z; P.min_pierced = min_pierced;
    P.use_fraction = use_fraction != 0; P.use_stamp = use_stamp != 0; P.use_box = use_box != 0; P.use_ratio = use_ratio != 0;
    const unsigned long long *keys = (const unsigned long long *)in_keys;
    const int grid = pcacc_grid(m, ACCR_BLOCK);
    hipLaunchKernelGGL(accr_reason_kernel, dim3(grid), dim3(ACCR_BLOCK), 0, st, keys, in_acc, in_stamps, in_pierced, in_capacity, m, P, t.flag, t.reason);
    pcacc_scan_i32(t.flag, m, t.chunk, t.kpos, st);                                               // kpos[m] = stage-A survivors
    PCACC_CHECK_LAUNCH();
    if (min_neighbors > 0) {
        hipLaunchKernelGGL(accr_dst_kernel, dim3(grid), dim3(ACCR_BLOCK), 0, st, (const int *)t.flag, (const int *)t.kpos, m, t.dst, t.rows);
        // a lane runs (2r+1)^2 serial searches: many small workgroups spread over the CUs, as accum_normals.hip
        hipLaunchKernelGGL(accr_isolated_kernel, dim3(pcacc_grid(m, ACCR_BLOCK, 1 << 22)), dim3(ACCR_BLOCK), 0, st, keys, m, (const int *)t.dst,
                           (const int *)t.rows, (const int *)(t.kpos + m), (int)radius, (int)min_neighbors, t.flag, t.reason);
        pcacc_scan_i32(t.flag, m, t.chunk, t.kpos, st);                                           // kpos[m] = survivors of both stages
        PCACC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(accr_compact_kernel, dim3(grid), dim3(ACCR_BLOCK), 0, st, keys, in_acc, in_stamps, in_pierced, in_capacity, m, (const int *)t.flag,
                       (const int *)t.kpos, (const uint8_t *)t.reason, dry_run != 0 ? 1 : 0, (unsigned long long *)out_keys, out_acc, out_stamps,
                       in_pierced ? out_pierced : (int32_t *)nullptr, out_capacity, (unsigned long long *)counters, state);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
