// C6. Scan-to-map point-to-plane registration against the accumulated scene cloud (include/pcacc.h C6).
//
// The map of accum.hip is a sorted key list, the normals of accum_normals.hip are rows of the kept voxels: a scan point finds its plane with nine
// column searches (accn_column, r = 1) and no other index.  No hash table, no floating-point atomics, no inline assembly.
//   rows     pass 1 of C5 (accn_rows_launch): dst[m], the row of the normal tables of every map row, -1 = filtered out.
//   count    eligible points (not flagged moving) and candidate rows (a valid normal), integer sums; accr_begin seeds the job's state from them and
//            ends the job at once when the normal tables do not have the rows the filter keeps.
//   corr     round k, one lane per scan point, one workgroup per slot of 256 points: accr_point of accum_register.h -- the code the host build runs
//            with every index assert-checked -- then the slot tree, value by value: 6 shuffle steps per wave, the 4 wave sums added left to right.
//   update   round k, one wave: the slot sums added in slot order, then accr_round on one lane: statistics, stop rule, 6x6 Cholesky, pose update.
// The stop is decided on the device: the host queues 2 (max_iter + 1) launches and never waits; a finished job's later rounds return at once.
// Everything a result depends on is added in an order the header fixes: two runs give the same bits.
#include "scan.h"
#include "accum_register.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCR_MAX_POINTS ((int64_t)1 << 24)          // 65 536 slots: the update wave adds them one after the other
#define ACCR_MAX_ITERATIONS 10000

struct AccrWs {
    AccnRows rows;
    double *partial;                                // [slots][ACCR_TERMS]
    AccrState *state;                               // | zero-filled per call
    unsigned long long *cnt;                        // | [4]: eligible, candidates, -, kept (pass 1's out_n)
    size_t zero_off, zero_bytes;
};

static int64_t accr_slots(int64_t n) { return (n + ACCR_SLOT - 1) / ACCR_SLOT; }

static size_t accr_carve(AccrWs *w, char *base, int64_t n, int64_t m)
{
    size_t off = accn_rows_carve(m > 0 ? m : 1, &w->rows, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    const int64_t slots = accr_slots(n);
    w->partial = (double *)take((size_t)(slots > 0 ? slots : 1) * ACCR_TERMS * 8);
    w->zero_off = off;
    w->state = (AccrState *)take(sizeof(AccrState));
    w->cnt = (unsigned long long *)take(4 * 8);
    w->zero_bytes = off - w->zero_off;
    return off;
}

static __global__ __launch_bounds__(256) void accr_count_kernel(const uint8_t *__restrict__ moving, int64_t n, const uint8_t *__restrict__ flags,
                                                                int64_t n_rows, unsigned long long *__restrict__ cnt)
{
    unsigned long long e = 0, c = 0;
    if (moving)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) e += moving[i] ? 0 : 1;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_rows; j += (int64_t)gridDim.x * 256)
        c += (flags[j] & (ACCN_FEW_NEIGHBORS | ACCN_DEGENERATE)) ? 0 : 1;
    for (int s = 32; s > 0; s >>= 1) { e += __shfl_down(e, s, 64); c += __shfl_down(c, s, 64); }
    if (lane_id() == 0) {                                                                    // integer sums: any order gives the same value
        if (e) atomicAdd(&cnt[0], e);
        if (c) atomicAdd(&cnt[1], c);
    }
}

static __global__ void accr_begin_kernel(const double *__restrict__ init, const uint8_t *moving, int64_t n, int64_t m, int64_t n_rows,
                                         const int *__restrict__ kpos, const unsigned long long *__restrict__ cnt, AccrState *st, AccrOut o)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    accr_init(st, init, moving ? (int64_t)cnt[0] : n, (int64_t)cnt[1]);
    const int64_t kept = m > 0 ? (int64_t)kpos[m] : 0;
    if (kept != n_rows) accr_finish(st, &o, st->T_good, 0.0, 0.0, 0, ACCR_BAD_TABLE, 0.0);   // the tables are of another filter: no round reads them
}

static __global__ __launch_bounds__(ACCR_SLOT) void accr_corr_kernel(const float *__restrict__ points, const uint8_t *__restrict__ moving, int64_t n,
                                                                      double voxel_size, double max_d2, const unsigned long long *__restrict__ keys,
                                                                      const int64_t *__restrict__ acc, int64_t capacity, int64_t m,
                                                                      const int *__restrict__ dst, const float *__restrict__ normals,
                                                                      const uint8_t *__restrict__ flags, int64_t n_rows, const AccrState *st,
                                                                      double *__restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double red[ACCR_SLOT / ACCR_GROUP][ACCR_TERMS];
    if (st->done) return;                                                                    // uniform over the workgroup
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = st->T[k];
    const int64_t i = (int64_t)blockIdx.x * ACCR_SLOT + threadIdx.x;
    double t[ACCR_TERMS];
    int64_t row;
    if (i < n) {
        accr_point(keys, acc, capacity, m, dst, normals, flags, n_rows, T, points, moving, n, i, voxel_size, max_d2, t, &row);
    } else {
        for (int k = 0; k < ACCR_TERMS; ++k) t[k] = 0.0;
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ACCR_TERMS; ++k) {                                                   // accr_slot_sum's tree, one value at a time
        double v = t[k];
#pragma unroll
        for (int s = ACCR_GROUP / 2; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
        if (lane_id() == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ACCR_TERMS) {
        double sum = red[0][threadIdx.x];
        for (int g = 1; g < ACCR_SLOT / ACCR_GROUP; ++g) sum = sum + red[g][threadIdx.x];
        partial[(int64_t)blockIdx.x * ACCR_TERMS + threadIdx.x] = sum;
    }
}

static __global__ __launch_bounds__(64) void accr_update_kernel(const double *__restrict__ partial, int64_t slots, int round, int max_iter, AccrState *st,
                                                                AccrOut o)
{
#pragma clang fp contract(off)
    __shared__ double sums[ACCR_TERMS];
    __shared__ double tile[64 * ACCR_TERMS];
    if (st->done) return;
    double v = 0.0;
    for (int64_t s0 = 0; s0 < slots; s0 += 64) {                                             // 64 slots at a time through LDS: the wave loads, 29 lanes add
        const int cnt = slots - s0 < 64 ? (int)(slots - s0) : 64;
        for (int e = threadIdx.x; e < cnt * ACCR_TERMS; e += 64) tile[e] = partial[s0 * ACCR_TERMS + e];
        __syncthreads();
        if (threadIdx.x < ACCR_TERMS)
            for (int s = 0; s < cnt; ++s) v = v + tile[s * ACCR_TERMS + threadIdx.x];        // slot order
        __syncthreads();
    }
    if (threadIdx.x < ACCR_TERMS) sums[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) accr_round(st, sums, round, max_iter, &o);
}

static bool accr_sizes_ok(int64_t n, int64_t m) { return n >= 0 && n <= ACCR_MAX_POINTS && m >= 0 && m <= ACCUM_MAX_CAPACITY; }

extern "C" int pcacc_accum_register_workspace_bytes(int64_t n, int64_t m, size_t *bytes)
{
    if (!bytes || !accr_sizes_ok(n, m)) return PCACC_E_ARG;
    AccrWs w;
    *bytes = accr_carve(&w, nullptr, n, m);
    return PCACC_OK;
}

extern "C" int pcacc_accum_register(const float *points, int64_t n, const uint8_t *moving, const double *init_pose, double voxel_size,
                                    double max_distance, int32_t max_iter, const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m,
                                    int64_t min_count, int32_t use_fraction, double max_moving_fraction, const float *normals, const uint8_t *flags,
                                    int64_t n_rows, double *out_pose, double *out_fitness, double *out_rmse, int32_t *out_iterations,
                                    int32_t *out_status, int32_t *out_correspondences, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!accr_sizes_ok(n, m) || capacity < m || capacity > ACCUM_MAX_CAPACITY || n_rows < 0 || n_rows > m) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size < 1e300) || !(max_distance > 0.0) || !(max_distance <= voxel_size)) return PCACC_E_ARG;
    if (max_iter < 0 || max_iter > ACCR_MAX_ITERATIONS) return PCACC_E_ARG;
    if (!out_pose || !out_fitness || !out_rmse || !out_iterations || !out_status || !out_correspondences || !workspace) return PCACC_E_ARG;
    if ((n > 0 && !points) || (m > 0 && (!keys || !acc)) || (n_rows > 0 && (!normals || !flags))) return PCACC_E_ARG;
    AccrWs w;
    if (workspace_bytes < accr_carve(&w, (char *)workspace, n, m)) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync((char *)workspace + w.zero_off, 0, w.zero_bytes, st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m > 0 && accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, (int64_t *)(w.cnt + 3), st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    const AccrOut o = {out_pose, out_fitness, out_rmse, out_iterations, out_status, out_correspondences};
    const int64_t count_items = (moving && n > n_rows) ? n : n_rows;
    if (count_items > 0)
        hipLaunchKernelGGL(accr_count_kernel, dim3(pcacc_grid(count_items, 256)), dim3(256), 0, st, moving, n, flags, n_rows, w.cnt);
    hipLaunchKernelGGL(accr_begin_kernel, dim3(1), dim3(1), 0, st, init_pose, moving, n, m, n_rows, (const int *)w.rows.kpos,
                       (const unsigned long long *)w.cnt, w.state, o);
    PCACC_CHECK_LAUNCH();
    const int64_t slots = (m > 0 && n_rows > 0) ? accr_slots(n) : 0;                         // without a table no point has a candidate
    const double max_d2 = max_distance * max_distance;
    for (int round = 0; round <= max_iter; ++round) {
        if (slots > 0)
            hipLaunchKernelGGL(accr_corr_kernel, dim3((unsigned)slots), dim3(ACCR_SLOT), 0, st, points, moving, n, voxel_size, max_d2,
                               (const unsigned long long *)keys, acc, capacity, m, (const int *)w.rows.dst, normals, flags, n_rows,
                               (const AccrState *)w.state, w.partial);
        hipLaunchKernelGGL(accr_update_kernel, dim3(1), dim3(64), 0, st, (const double *)w.partial, slots, round, (int)max_iter, w.state, o);
    }
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
