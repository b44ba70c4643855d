// C15. Two tables of observed space into one, and a table under a rigid pose and / or a new voxel size (include/pcacc.h C15).
//
//   merge    M0 begin     the state words of both tables against ma and mb
//            M1 search    every B row binary-searched in A's keys: hit or miss, and its position (accm_search of C12)
//            M2 scan      scan.h over the misses -> mrank, mrank[nb] = keys of B that A lacks
//            M3 decide    one thread: ma + misses against the capacity of the output tables -> counters, state (accom_decide); NOTHING has touched a
//                         table so far
//            M4 old rows  A row p -> p + mrank[lower bound of its key in B], plus B's row when B holds the key (accom_old_row)
//            M5 new rows  missed B row j -> position + mrank[j], copied (accom_new_row).  Out of place: A and B stay as they were.  No atomic anywhere.
//   regrid   G0 begin     the state words against m
//            G1 keys      key (or the all-ones invalid key, which sorts to the end) and row number of every table row under the pose (accog_row)
//            G2 rocPRIM   radix sort of (key, row) on 64 bits
//            G3 heads     run heads of the sorted keys, scan.h -> output row of every sorted position, rows of the new table
//            G4 clear     the rows of the new table: rays 0, stamps INT32_MAX / INT32_MIN
//            G5 reduce    a segmented max / min / max over the 64 lanes of a wave, then ONE integer atomicMax / atomicMin per (wave, run) and column.
//                         Integer max and min commute: the result is bit-identical from run to run.
//            G6 finish    counters and the sixteen state words of the new table
// The functions are those the host build runs with every index assert-checked.  No floating-point atomics, no LDS beyond the scan's, no inline
// assembly; nothing is read back.
#include <rocprim/device/device_radix_sort.hpp>

#include "scan.h"
#include "accum_observe_merge.h"
#include "accum_launch.h"

#define ACCOM_BLOCK 256

static_assert(ACCOM_STATE_WORDS == PCACC_OBSERVE_STATE_WORDS && ACCOM_NUM_VOXELS == PCACC_OBSERVE_NUM_VOXELS && ACCOM_STATUS == PCACC_OBSERVE_STATUS &&
              ACCOM_NEEDED == PCACC_OBSERVE_NEEDED && ACCOM_NEEDED_VISITS == PCACC_OBSERVE_NEEDED_VISITS && ACCOM_CALL_VISITS == PCACC_OBSERVE_CALL_VISITS &&
              ACCOM_CALL_VOXELS == PCACC_OBSERVE_CALL_VOXELS && ACCOM_WALKED == PCACC_OBSERVE_WALKED && PCACC_OBSERVE_VISITS == PCACC_OBSERVE_WALKED + 4,
              "accum_observe_merge.h restates the state words of include/pcacc.h");
static_assert(ACCOM_C_STATUS == PCACC_OBSERVED_MERGE_STATUS && ACCOM_C_NEEDED == PCACC_OBSERVED_MERGE_NEEDED && ACCOM_C_SHARED == PCACC_OBSERVED_MERGE_SHARED &&
              ACCOM_C_NEW == PCACC_OBSERVED_MERGE_NEW && PCACC_OBSERVED_MERGE_COUNTERS == 4 && ACCOG_C_ROWS_IN == PCACC_OBSERVED_REGRID_ROWS_IN &&
              ACCOG_C_ROWS_OUT == PCACC_OBSERVED_REGRID_ROWS_OUT && ACCOG_C_DROPPED_ROWS == PCACC_OBSERVED_REGRID_DROPPED_ROWS &&
              PCACC_OBSERVED_REGRID_COUNTERS == 3, "accum_observe_merge.h restates the counters of include/pcacc.h");

struct AccomHdr { long long total; int go; int bad; };

// ---- merge -------------------------------------------------------------------------------------------------------------------------------------------
// M0.  state and b_state may be the same words.
static __global__ void accom_begin_kernel(const int64_t *state, int64_t ma, const int64_t *b_state, int64_t mb, AccomHdr *hdr)
{
    hdr->bad = accom_state_fits(state, ma, b_state, mb) ? 0 : 1;
    hdr->go = 0;
    hdr->total = 0;
}

// M1.  miss[j] = 0 for j past B's rows, so that the scan may run over nb >= 1 entries.  With state words that do not fit, no table is addressed.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accom_search_kernel(const unsigned long long *__restrict__ a_keys, int64_t ma,
                                                                           const unsigned long long *__restrict__ b_keys, int64_t mb, int64_t nb,
                                                                           const AccomHdr *hdr, int *__restrict__ miss, int *__restrict__ pos)
{
    const bool bad = hdr->bad != 0;
    for (int64_t j = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; j < nb; j += (int64_t)gridDim.x * ACCOM_BLOCK) {
        int64_t p = 0;
        miss[j] = bad ? 0 : accm_search(a_keys, ma, b_keys, mb, j, &p);
        pos[j] = (int)p;
    }
}

// M3.
static __global__ void accom_decide_kernel(int64_t *counters, int64_t *state, const int64_t *b_state, AccomHdr *hdr, const int *mrank, int64_t ma,
                                           int64_t mb, int64_t nb, int64_t out_capacity)
{
    const long long fresh = mrank[nb];
    const int status = accom_decide(hdr->bad != 0, ma, mb, fresh, out_capacity, b_state, state, counters);
    hdr->total = ma + fresh;
    hdr->go = status == ACCO_OK;
}

// M4.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accom_old_kernel(const unsigned long long *__restrict__ a_keys, const int64_t *__restrict__ a_rays,
                                                                        const int32_t *__restrict__ a_stamps, int64_t a_capacity, int64_t ma,
                                                                        const unsigned long long *__restrict__ b_keys, const int64_t *__restrict__ b_rays,
                                                                        const int32_t *__restrict__ b_stamps, int64_t b_capacity, int64_t mb,
                                                                        const int *__restrict__ mrank, int64_t nb, unsigned long long *__restrict__ out_keys,
                                                                        int64_t *__restrict__ out_rays, int32_t *__restrict__ out_stamps,
                                                                        int64_t out_capacity, const AccomHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total;
    for (int64_t p = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; p < ma; p += (int64_t)gridDim.x * ACCOM_BLOCK) {
        int shared;
        accom_old_row(a_keys, a_rays, a_stamps, a_capacity, ma, b_keys, b_rays, b_stamps, b_capacity, mb, mrank, nb + 1, p, out_keys, out_rays, out_stamps,
                      out_capacity, total, &shared);
    }
}

// M5.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accom_new_kernel(const unsigned long long *__restrict__ b_keys, const int64_t *__restrict__ b_rays,
                                                                        const int32_t *__restrict__ b_stamps, int64_t b_capacity, int64_t mb,
                                                                        const int *__restrict__ miss, const int *__restrict__ pos,
                                                                        const int *__restrict__ mrank, int64_t nb, unsigned long long *__restrict__ out_keys,
                                                                        int64_t *__restrict__ out_rays, int32_t *__restrict__ out_stamps,
                                                                        int64_t out_capacity, const AccomHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total;
    for (int64_t j = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; j < mb; j += (int64_t)gridDim.x * ACCOM_BLOCK) {
        if (!miss[j]) continue;
        accom_new_row(b_keys, b_rays, b_stamps, b_capacity, mb, mrank, nb + 1, j, pos[j], out_keys, out_rays, out_stamps, out_capacity, total);
    }
}

struct AccomWs { AccomHdr *hdr; int *miss, *pos, *mrank, *chunk; };

static size_t accom_carve(int64_t nb, AccomWs *w, char *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->hdr = (AccomHdr *)take(sizeof(AccomHdr));
    w->miss = (int *)take((size_t)nb * 4);
    w->pos = (int *)take((size_t)nb * 4);
    w->mrank = (int *)take((size_t)(nb + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(nb) * 4);
    return off;
}

// The three tables of one side against the three of the other through accum_bytes_overlap: some pair shares a byte.
static bool accom_tables_share(const void *in_keys, const void *in_rays, const void *in_stamps, int64_t in_capacity, const void *out_keys,
                                 const void *out_rays, const void *out_stamps, int64_t out_capacity)
{
    const void *in_tab[3] = {in_keys, in_rays, in_stamps}, *out_tab[3] = {out_keys, out_rays, out_stamps};
    for (int a = 0; a < 3; ++a)                                                  // every table is 8 bytes per row
        for (int b = 0; b < 3; ++b)
            if (accum_bytes_overlap(in_tab[a], 8 * (size_t)in_capacity, out_tab[b], 8 * (size_t)out_capacity)) return true;
    return false;
}

extern "C" int pcacc_accum_observed_merge_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes)
{
    if (!bytes || ma < 0 || ma > ACCUM_MAX_CAPACITY || mb < 0 || mb > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccomWs w;
    *bytes = accom_carve(mb > 0 ? mb : 1, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_observed_merge(const int64_t *a_keys, const int64_t *a_rays, const int32_t *a_stamps, int64_t a_capacity, int64_t ma,
                                          const int64_t *b_keys, const int64_t *b_rays, const int32_t *b_stamps, int64_t b_capacity, int64_t mb,
                                          const int64_t *b_state, int64_t *out_keys, int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity,
                                          int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes, void *stream)
{
    if (a_capacity < 0 || a_capacity > ACCUM_MAX_CAPACITY || b_capacity < 0 || b_capacity > ACCUM_MAX_CAPACITY || out_capacity < 0 ||
        out_capacity > ACCUM_MAX_CAPACITY)
        return PCACC_E_ARG;
    if (ma < 0 || ma > a_capacity || mb < 0 || mb > b_capacity || !counters || !state || !b_state) return PCACC_E_ARG;
    if (ma > 0 && (!a_keys || !a_rays || !a_stamps)) return PCACC_E_ARG;
    if (mb > 0 && (!b_keys || !b_rays || !b_stamps)) return PCACC_E_ARG;
    if (out_capacity > 0 && (!out_keys || !out_rays || !out_stamps)) return PCACC_E_ARG;
    if (accom_tables_share(a_keys, a_rays, a_stamps, a_capacity, out_keys, out_rays, out_stamps, out_capacity) ||
        accom_tables_share(b_keys, b_rays, b_stamps, b_capacity, out_keys, out_rays, out_stamps, out_capacity))
        return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (ma == 0 && mb == 0) {
        if (hipMemsetAsync(counters, 0, PCACC_OBSERVED_MERGE_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
        return PCACC_OK;
    }
    if (!workspace) return PCACC_E_ARG;
    const int64_t nb = mb > 0 ? mb : 1;
    AccomWs w;
    if (workspace_bytes < accom_carve(nb, &w, (char *)workspace)) return PCACC_E_WORKSPACE;
    const unsigned long long *ak = (const unsigned long long *)a_keys, *bk = (const unsigned long long *)b_keys;
    hipLaunchKernelGGL(accom_begin_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)state, ma, b_state, mb, w.hdr);
    hipLaunchKernelGGL(accom_search_kernel, dim3(pcacc_grid(nb, ACCOM_BLOCK)), dim3(ACCOM_BLOCK), 0, st, ak, ma, bk, mb, nb, (const AccomHdr *)w.hdr, w.miss,
                       w.pos);
    PCACC_CHECK_LAUNCH();
    pcacc_scan_i32(w.miss, nb, w.chunk, w.mrank, st);                                             // mrank[nb] = keys of B that A lacks
    hipLaunchKernelGGL(accom_decide_kernel, dim3(1), dim3(1), 0, st, counters, state, b_state, w.hdr, (const int *)w.mrank, ma, mb, nb, out_capacity);
    PCACC_CHECK_LAUNCH();
    if (ma > 0)
        hipLaunchKernelGGL(accom_old_kernel, dim3(pcacc_grid(ma, ACCOM_BLOCK)), dim3(ACCOM_BLOCK), 0, st, ak, a_rays, a_stamps, a_capacity, ma, bk, b_rays,
                           b_stamps, b_capacity, mb, (const int *)w.mrank, nb, (unsigned long long *)out_keys, out_rays, out_stamps, out_capacity,
                           (const AccomHdr *)w.hdr);
    if (mb > 0)
        hipLaunchKernelGGL(accom_new_kernel, dim3(pcacc_grid(mb, ACCOM_BLOCK)), dim3(ACCOM_BLOCK), 0, st, bk, b_rays, b_stamps, b_capacity, mb,
                           (const int *)w.miss, (const int *)w.pos, (const int *)w.mrank, nb, (unsigned long long *)out_keys, out_rays, out_stamps,
                           out_capacity, (const AccomHdr *)w.hdr);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// ---- regrid ------------------------------------------------------------------------------------------------------------------------------------------
// G0.
static __global__ void accog_begin_kernel(const int64_t *in_state, int64_t m, AccomHdr *hdr)
{
    hdr->bad = in_state[ACCOM_NUM_VOXELS] == m ? 0 : 1;
    hdr->go = 0;
    hdr->total = 0;
}

// G1.  With state words that do not fit, every key is the invalid one and no table is addressed: the passes behind this one find no run.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accog_keys_kernel(const unsigned long long *__restrict__ keys, int64_t capacity, int64_t m,
                                                                         const double *__restrict__ pose, double in_voxel_size, double out_voxel_size,
                                                                         const AccomHdr *hdr, unsigned long long *__restrict__ key_out,
                                                                         int *__restrict__ idx_out, unsigned long long *__restrict__ counters)
{
    double T[16];
    pcacc_pose_seed(T, pose);                                                    // NULL = identity, through the same arithmetic
    const bool bad = hdr->bad != 0;
    long long dropped = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCOM_BLOCK) {
        unsigned long long key = ACC_INVALID_KEY;
        if (!bad && !accog_row(keys, capacity, m, i, T, in_voxel_size, out_voxel_size, &key)) {
            key = ACC_INVALID_KEY;
            ++dropped;
        }
        key_out[i] = key;
        idx_out[i] = (int)i;
    }
    accum_wave_count(counters, PCACC_OBSERVED_REGRID_DROPPED_ROWS, dropped);     // every lane of the wave arrives here
}

// G3.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accog_heads_kernel(const unsigned long long *__restrict__ sorted, int64_t m, int *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCOM_BLOCK) head[i] = accog_head(sorted, i, m);
}

// G4.  runs <= m <= out_capacity.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accog_clear_kernel(const int *__restrict__ runs_ptr, int64_t m, int64_t *__restrict__ out_rays,
                                                                          int32_t *__restrict__ out_stamps, int64_t out_capacity)
{
    int64_t runs = *runs_ptr;
    if (runs > m) runs = m;
    for (int64_t e = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; e < runs; e += (int64_t)gridDim.x * ACCOM_BLOCK) {
        out_rays[e] = 0;
        out_stamps[e] = INT32_MAX;
        out_stamps[out_capacity + e] = INT32_MIN;
    }
}

// The segmented fold over the 64 lanes of a wave: lane's record folded (accog_fold) with those of the lanes before it in the same run r.
static __device__ __forceinline__ void accog_seg_fold(long long *rays, int *t0, int *t1, int r, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long ry = __shfl_up(*rays, d, 64);
        const int a = __shfl_up(*t0, d, 64), b = __shfl_up(*t1, d, 64);
        const int rr = __shfl_up(r, d, 64);
        if (lane >= d && rr == r) {                                              // r ascends along the lanes: equal at distance d = equal all the way
            int64_t v = *rays;
            int32_t u0 = *t0, u1 = *t1;
            accog_fold(&v, &u0, &u1, ry, a, b);
            *rays = v; *t0 = u0; *t1 = u1;
        }
    }
}

// G5.  A wave takes 64 consecutive sorted positions per pass; all 64 lanes stay in the loop (the bound is wave-uniform).  A ray count is >= 0, so the
// unsigned 64-bit atomicMax orders it as the signed comparison does.
static __global__ __launch_bounds__(ACCOM_BLOCK) void accog_reduce_kernel(const int64_t *__restrict__ rays, const int32_t *__restrict__ stamps,
                                                                           int64_t capacity, int64_t m, const unsigned long long *__restrict__ sorted,
                                                                           const int *__restrict__ idx, const int *__restrict__ head,
                                                                           const int *__restrict__ vox, unsigned long long *__restrict__ out_keys,
                                                                           int64_t *__restrict__ out_rays, int32_t *__restrict__ out_stamps,
                                                                           int64_t out_capacity)
{
    int64_t runs = vox[m];
    if (runs > m) runs = m;
    const int lane = lane_id();
    const int64_t m_pad = (m + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * ACCOM_BLOCK + threadIdx.x; i < m_pad; i += (int64_t)gridDim.x * ACCOM_BLOCK) {
        int r = -1;
        long long ry = 0;
        int t0 = INT32_MAX, t1 = INT32_MIN;
        if (i < m) {
            int64_t row;
            const int64_t run = accog_position(sorted, idx, head, vox, m, runs, i, &row);
            if (run >= 0 && row >= 0 && m <= capacity) {
                r = (int)run;
                ry = rays[row];
                t0 = stamps[row]; t1 = stamps[capacity + row];
                if (head[i]) out_keys[run] = sorted[i];
            }
        }
        accog_seg_fold(&ry, &t0, &t1, r, lane);
        const int r_next = __shfl_down(r, 1, 64);
        if (r >= 0 && (lane == 63 || r_next != r)) {                             // last lane of its run in this wave
            if (ry > 0) atomicMax((unsigned long long *)&out_rays[r], (unsigned long long)ry);
            atomicMin(&out_stamps[r], t0);
            atomicMax(&out_stamps[out_capacity + r], t1);
        }
    }
}

// G6.  runs_ptr = NULL: an empty table.  On state words that do not fit, out_state[STATUS] is the only word written (the counters stay zero).
static __global__ void accog_finish_kernel(const int *runs_ptr, int64_t m, const int64_t *in_state, const AccomHdr *hdr, int64_t *counters,
                                           int64_t *out_state)
{
    if (hdr ? hdr->bad != 0 : in_state[ACCOM_NUM_VOXELS] != m) {
        out_state[ACCOM_STATUS] = ACCO_BAD_STATE;
        return;
    }
    int64_t runs = runs_ptr ? *runs_ptr : 0;
    if (runs > m) runs = m;
    counters[PCACC_OBSERVED_REGRID_ROWS_IN] = m;
    counters[PCACC_OBSERVED_REGRID_ROWS_OUT] = runs;
    accog_state(in_state, runs, out_state);
}

struct AccogWs {
    AccomHdr *hdr;
    unsigned long long *key_a, *key_b;
    int *idx_a, *idx_b, *head, *vox, *chunk;
    void *sort_tmp;
    size_t sort_tmp_bytes, total;
};

static int accog_carve(int64_t n, char *base, AccogWs *w)
{
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
        return PCACC_E_LAUNCH;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    const size_t un = (size_t)n;
    w->hdr = (AccomHdr *)take(sizeof(AccomHdr));
    w->key_a = (unsigned long long *)take(un * 8);
    w->key_b = (unsigned long long *)take(un * 8);
    w->idx_a = (int *)take(un * 4);
    w->idx_b = (int *)take(un * 4);
    w->head = (int *)take(un * 4);
    w->vox = (int *)take((un + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(n) * 4);
    w->sort_tmp = take(sort_bytes);
    w->sort_tmp_bytes = sort_bytes;
    w->total = off;
    return PCACC_OK;
}

extern "C" int pcacc_accum_observed_regrid_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccogWs w;
    const int rc = accog_carve(m > 0 ? m : 1, nullptr, &w);
    if (rc != PCACC_OK) return rc;
    *bytes = w.total;
    return PCACC_OK;
}

extern "C" int pcacc_accum_observed_regrid(const int64_t *in_keys, const int64_t *in_rays, const int32_t *in_stamps, int64_t in_capacity, int64_t m,
                                           const int64_t *in_state, const double *pose, double in_voxel_size, double out_voxel_size, int64_t *out_keys,
                                           int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity, int64_t *counters, int64_t *out_state,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || in_capacity < m || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < m || out_capacity > ACCUM_MAX_CAPACITY || !counters || !in_state ||
        !out_state)
        return PCACC_E_ARG;
    if (!(in_voxel_size > 0.0) || !(in_voxel_size - in_voxel_size == 0.0) || !(out_voxel_size > 0.0) || !(out_voxel_size - out_voxel_size == 0.0))
        return PCACC_E_ARG;
    if (m > 0 && (!in_keys || !in_rays || !in_stamps || !out_keys || !out_rays || !out_stamps || !workspace)) return PCACC_E_ARG;
    if (accom_tables_share(in_keys, in_rays, in_stamps, in_capacity, out_keys, out_rays, out_stamps, out_capacity)) return PCACC_E_ARG;
    AccogWs w;
    if (m > 0) {
        const int rc = accog_carve(m, (char *)workspace, &w);
        if (rc != PCACC_OK) return rc;
        if (workspace_bytes < w.total) return PCACC_E_WORKSPACE;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, PCACC_OBSERVED_REGRID_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) {
        hipLaunchKernelGGL(accog_finish_kernel, dim3(1), dim3(1), 0, st, (const int *)nullptr, m, in_state, (const AccomHdr *)nullptr, counters, out_state);
        PCACC_CHECK_LAUNCH();
        return PCACC_OK;
    }
    const int grid = pcacc_grid(m, ACCOM_BLOCK);
    hipLaunchKernelGGL(accog_begin_kernel, dim3(1), dim3(1), 0, st, in_state, m, w.hdr);
    hipLaunchKernelGGL(accog_keys_kernel, dim3(grid), dim3(ACCOM_BLOCK), 0, st, (const unsigned long long *)in_keys, in_capacity, m, pose, in_voxel_size,
                       out_voxel_size, (const AccomHdr *)w.hdr, w.key_a, w.idx_a, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    if (rocprim::radix_sort_pairs(w.sort_tmp, w.sort_tmp_bytes, w.key_a, w.key_b, w.idx_a, w.idx_b, (size_t)m, 0, 64, st) != hipSuccess)
        return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(accog_heads_kernel, dim3(grid), dim3(ACCOM_BLOCK), 0, st, (const unsigned long long *)w.key_b, m, w.head);
    pcacc_scan_i32(w.head, m, w.chunk, w.vox, st);                                                // vox[m] = rows of the new table
    hipLaunchKernelGGL(accog_clear_kernel, dim3(grid), dim3(ACCOM_BLOCK), 0, st, (const int *)(w.vox + m), m, out_rays, out_stamps, out_capacity);
    hipLaunchKernelGGL(accog_reduce_kernel, dim3(grid), dim3(ACCOM_BLOCK), 0, st, in_rays, in_stamps, in_capacity, m, (const unsigned long long *)w.key_b,
                       (const int *)w.idx_b, (const int *)w.head, (const int *)w.vox, (unsigned long long *)out_keys, out_rays, out_stamps, out_capacity);
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accog_finish_kernel, dim3(1), dim3(1), 0, st, (const int *)(w.vox + m), m, in_state, (const AccomHdr *)w.hdr, counters, out_state);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
