// C12. Two accumulated scene clouds into one, and a map under a rigid pose and / or a new voxel size (include/pcacc.h C12).
//
//   merge    M1 search    every B row binary-searched in A's keys: hit or miss, and its position (accm_search)
//            M2 scan      scan.h over the misses -> mrank, mrank[nb] = keys of B that A lacks
//            M3 decide    one thread: ma + misses against the capacity of the output tables -> counters, state; NOTHING has touched a table so far
//            M4 old rows  A row p -> p + mrank[lower bound of its key in B], plus B's record when B holds the key (accm_old_row)
//            M5 new rows  missed B row j -> position + mrank[j], copied (accm_new_row).  Out of place: A and B stay as they were.
//   regrid   G1 keys      key (or the all-ones invalid key, which sorts to the end) and row number of every map row under the pose (accg_row)
//            G2 rocPRIM   radix sort of (key, row) on 64 bits
//            G3 heads     run heads of the sorted keys, scan.h -> output row of every sorted position, rows of the new map
//            G4 clear     the rows of the new map: sums 0, stamps INT32_MAX / INT32_MIN
//            G5 reduce    the contributions (recomputed from the row with the arithmetic of G1) summed per run: a segmented scan over the 64 lanes
//                         of a wave, then ONE 64-bit integer atomic per (wave, run) and field, 32-bit integer atomic min / max for the stamps
//            G6 finish    ray counts clamped, counters and the eight state words of the new map
// The functions are those the host build runs with every index assert-checked.  No floating-point atomics, no LDS beyond the scan's, no inline
// assembly; nothing is read back.
#include <rocprim/device/device_radix_sort.hpp>

#include "scan.h"
#include "accum_merge.h"
#include "accum_launch.h"

#define ACCM_BLOCK 256

struct AccmHdr { long long total; int go; };

// ---- merge -------------------------------------------------------------------------------------------------------------------------------------------
// M1.  miss[j] = 0 for j past B's rows, so that the scan may run over nb >= 1 entries.
static __global__ __launch_bounds__(ACCM_BLOCK) void accm_search_kernel(const unsigned long long *__restrict__ a_keys, int64_t ma,
                                                                         const unsigned long long *__restrict__ b_keys, int64_t mb, int64_t nb,
                                                                         int *__restrict__ miss, int *__restrict__ pos)
{
    for (int64_t j = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; j < nb; j += (int64_t)gridDim.x * ACCM_BLOCK) {
        int64_t p;
        miss[j] = accm_search(a_keys, ma, b_keys, mb, j, &p);
        pos[j] = (int)p;
    }
}

// M3.
static __global__ void accm_decide_kernel(int64_t *counters, int64_t *state, AccmHdr *hdr, const int *mrank, int64_t ma, int64_t mb, int64_t nb,
                                          int64_t out_capacity, int64_t add_dropped)
{
    const long long fresh = mrank[nb], total = ma + fresh;
    hdr->total = total;
    counters[PCACC_MERGE_NEEDED] = total;
    counters[PCACC_MERGE_SHARED] = mb - fresh;
    counters[PCACC_MERGE_NEW] = fresh;
    counters[PCACC_MERGE_SATURATED] = 0;
    if (total > out_capacity) { counters[PCACC_MERGE_STATUS] = PCACC_ACCUM_TOO_SMALL; hdr->go = 0; }
    else {
        counters[PCACC_MERGE_STATUS] = PCACC_ACCUM_OK;
        state[PCACC_ACCUM_NUM_VOXELS] = total;
        state[PCACC_ACCUM_DROPPED] += add_dropped;
        hdr->go = 1;
    }
}

// M4.
static __global__ __launch_bounds__(ACCM_BLOCK) void accm_old_kernel(const unsigned long long *__restrict__ a_keys, const int64_t *__restrict__ a_acc,
                                                                      const int32_t *__restrict__ a_stamps, const int32_t *__restrict__ a_pierced,
                                                                      int64_t a_capacity, int64_t ma, const unsigned long long *__restrict__ b_keys,
                                                                      const int64_t *__restrict__ b_acc, const int32_t *__restrict__ b_stamps,
                                                                      const int32_t *__restrict__ b_pierced, int64_t b_capacity, int64_t mb,
                                                                      const int *__restrict__ mrank, int64_t nb, unsigned long long *__restrict__ out_keys,
                                                                      int64_t *__restrict__ out_acc, int32_t *__restrict__ out_stamps,
                                                                      int32_t *__restrict__ out_pierced, int64_t out_capacity, const AccmHdr *hdr,
                                                                      unsigned long long *__restrict__ counters)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total;
    long long saturated = 0;
    for (int64_t p = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; p < ma; p += (int64_t)gridDim.x * ACCM_BLOCK) {
        const int flags = accm_old_row(a_keys, a_acc, a_stamps, a_pierced, a_capacity, ma, b_keys, b_acc, b_stamps, b_pierced, b_capacity, mb, mrank, nb + 1,
                                       p, out_keys, out_acc, out_stamps, out_pierced, out_capacity, total);
        saturated += (flags & ACCM_SATURATED) != 0;
    }
    accum_wave_count(counters, PCACC_MERGE_SATURATED, saturated);                // every lane of the wave arrives here
}

// M5.
static __global__ __launch_bounds__(ACCM_BLOCK) void accm_new_kernel(const unsigned long long *__restrict__ b_keys, const int64_t *__restrict__ b_acc,
                                                                      const int32_t *__restrict__ b_stamps, const int32_t *__restrict__ b_pierced,
                                                                      int64_t b_capacity, int64_t mb, const int *__restrict__ miss,
                                                                      const int *__restrict__ pos, const int *__restrict__ mrank, int64_t nb,
                                                                      unsigned long long *__restrict__ out_keys, int64_t *__restrict__ out_acc,
                                                                      int32_t *__restrict__ out_stamps, int32_t *__restrict__ out_pierced,
                                                                      int64_t out_capacity, const AccmHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total;
    for (int64_t j = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; j < mb; j += (int64_t)gridDim.x * ACCM_BLOCK) {
        if (!miss[j]) continue;
        accm_new_row(b_keys, b_acc, b_stamps, b_pierced, b_capacity, mb, mrank, nb + 1, j, pos[j], out_keys, out_acc, out_stamps, out_pierced, out_capacity,
                     total);
    }
}

struct AccmWs { AccmHdr *hdr; int *miss, *pos, *mrank, *chunk; };

static size_t accm_carve(int64_t nb, AccmWs *w, char *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->hdr = (AccmHdr *)take(sizeof(AccmHdr));
    w->miss = (int *)take((size_t)nb * 4);
    w->pos = (int *)take((size_t)nb * 4);
    w->mrank = (int *)take((size_t)(nb + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(nb) * 4);
    return off;
}

extern "C" int pcacc_accum_merge_workspace_bytes(int64_t ma, int64_t mb, size_t *bytes)
{
    if (!bytes || ma < 0 || ma > ACCUM_MAX_CAPACITY || mb < 0 || mb > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccmWs w;
    *bytes = accm_carve(mb > 0 ? mb : 1, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_merge(const int64_t *a_keys, const int64_t *a_acc, const int32_t *a_stamps, const int32_t *a_pierced, int64_t a_capacity,
                                 int64_t ma, const int64_t *b_keys, const int64_t *b_acc, const int32_t *b_stamps, const int32_t *b_pierced,
                                 int64_t b_capacity, int64_t mb, int64_t add_dropped, int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps,
                                 int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state, void *workspace, size_t workspace_bytes,
                                 void *stream)
{
    if (a_capacity < 0 || a_capacity > ACCUM_MAX_CAPACITY || b_capacity < 0 || b_capacity > ACCUM_MAX_CAPACITY || out_capacity < 0 ||
        out_capacity > ACCUM_MAX_CAPACITY)
        return PCACC_E_ARG;
    if (ma < 0 || ma > a_capacity || mb < 0 || mb > b_capacity || !counters || !state) return PCACC_E_ARG;
    if (ma > 0 && (!a_keys || !a_acc || !a_stamps)) return PCACC_E_ARG;
    if (mb > 0 && (!b_keys || !b_acc || !b_stamps)) return PCACC_E_ARG;
    const bool sidecar = a_pierced || b_pierced;
    if (out_capacity > 0 && (!out_keys || !out_acc || !out_stamps || (sidecar && !out_pierced))) return PCACC_E_ARG;
    if (accum_tables_overlap(a_keys, a_acc, a_stamps, a_pierced, a_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity) ||
        accum_tables_overlap(b_keys, b_acc, b_stamps, b_pierced, b_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity))
        return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (ma == 0 && mb == 0) {
        if (hipMemsetAsync(counters, 0, PCACC_MERGE_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
        if (hipMemsetAsync(state + PCACC_ACCUM_NUM_VOXELS, 0, sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
        return PCACC_OK;
    }
    if (!workspace) return PCACC_E_ARG;
    const int64_t nb = mb > 0 ? mb : 1;
    AccmWs w;
    if (workspace_bytes < accm_carve(nb, &w, (char *)workspace)) return PCACC_E_WORKSPACE;
    const unsigned long long *ak = (const unsigned long long *)a_keys, *bk = (const unsigned long long *)b_keys;
    int32_t *op = sidecar ? out_pierced : (int32_t *)nullptr;
    hipLaunchKernelGGL(accm_search_kernel, dim3(pcacc_grid(nb, ACCM_BLOCK)), dim3(ACCM_BLOCK), 0, st, ak, ma, bk, mb, nb, w.miss, w.pos);
    pcacc_scan_i32(w.miss, nb, w.chunk, w.mrank, st);                                             // mrank[nb] = keys of B that A lacks
    hipLaunchKernelGGL(accm_decide_kernel, dim3(1), dim3(1), 0, st, counters, state, w.hdr, (const int *)w.mrank, ma, mb, nb, out_capacity, add_dropped);
    PCACC_CHECK_LAUNCH();
    if (ma > 0)
        hipLaunchKernelGGL(accm_old_kernel, dim3(pcacc_grid(ma, ACCM_BLOCK)), dim3(ACCM_BLOCK), 0, st, ak, a_acc, a_stamps, a_pierced, a_capacity, ma, bk,
                           b_acc, b_stamps, b_pierced, b_capacity, mb, (const int *)w.mrank, nb, (unsigned long long *)out_keys, out_acc, out_stamps, op,
                           out_capacity, (const AccmHdr *)w.hdr, (unsigned long long *)counters);
    if (mb > 0)
        hipLaunchKernelGGL(accm_new_kernel, dim3(pcacc_grid(mb, ACCM_BLOCK)), dim3(ACCM_BLOCK), 0, st, bk, b_acc, b_stamps, b_pierced, b_capacity, mb,
                           (const int *)w.miss, (const int *)w.pos, (const int *)w.mrank, nb, (unsigned long long *)out_keys, out_acc, out_stamps, op,
                           out_capacity, (const AccmHdr *)w.hdr);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// ---- regrid ------------------------------------------------------------------------------------------------------------------------------------------
// G1.
static __global__ __launch_bounds__(ACCM_BLOCK) void accg_keys_kernel(const int64_t *__restrict__ acc, int64_t capacity, int64_t m,
                                                                       const double *__restrict__ pose, double out_voxel_size,
                                                                       unsigned long long *__restrict__ key_out, int *__restrict__ idx_out,
                                                                       unsigned long long *__restrict__ counters)
{
    double T[16];
    pcacc_pose_seed(T, pose);                                                    // NULL = identity, through the same arithmetic
    long long rows = 0, points = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCM_BLOCK) {
        unsigned long long key;
        int64_t term[ACC_FIELDS], count;
        if (!accg_row(acc, capacity, m, i, T, out_voxel_size, &key, term, &count)) {
            key = ACC_INVALID_KEY;
            ++rows;
            points += count > 0 ? count : 0;
        }
        key_out[i] = key;
        idx_out[i] = (int)i;
    }
    accum_wave_count(counters, PCACC_REGRID_DROPPED_ROWS, rows);
    accum_wave_count(counters, PCACC_REGRID_DROPPED_POINTS, points);
}

// G3.
static __global__ __launch_bounds__(ACCM_BLOCK) void accg_heads_kernel(const unsigned long long *__restrict__ keys, int64_t n, int *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCM_BLOCK) {
        const unsigned long long k = keys[i];
        head[i] = (k != ACC_INVALID_KEY && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
    }
}

// G4.  runs <= m <= out_capacity.
static __global__ __launch_bounds__(ACCM_BLOCK) void accg_clear_kernel(const int *__restrict__ runs_ptr, int64_t m, int64_t *__restrict__ out_acc,
                                                                        int32_t *__restrict__ out_stamps, int64_t out_capacity, long long *__restrict__ rays)
{
    int64_t runs = *runs_ptr;
    if (runs > m) runs = m;
    for (int64_t e = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; e < runs; e += (int64_t)gridDim.x * ACCM_BLOCK) {
#pragma unroll
        for (int f = 0; f < ACC_FIELDS; ++f) out_acc[accum_field(f, e, out_capacity)] = 0;
        out_stamps[e] = INT32_MAX;
        out_stamps[out_capacity + e] = INT32_MIN;
        rays[e] = 0;
    }
}

static __device__ __forceinline__ int accg_seg_min(int v, int r, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        const int rr = __shfl_up(r, d, 64);
        if (lane >= d && rr == r && t < v) v = t;
    }
    return v;
}

static __device__ __forceinline__ int accg_seg_max(int v, int r, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        const int rr = __shfl_up(r, d, 64);
        if (lane >= d && rr == r && t > v) v = t;
    }
    return v;
}

// G5.  A wave takes 64 consecutive sorted positions per pass; all 64 lanes stay in the loop (the bound is wave-uniform).
static __global__ __launch_bounds__(ACCM_BLOCK) void accg_reduce_kernel(const int64_t *__restrict__ acc, const int32_t *__restrict__ stamps,
                                                                         const int32_t *__restrict__ pierced, int64_t capacity, int64_t m,
                                                                         const double *__restrict__ pose, double out_voxel_size,
                                                                         const unsigned long long *__restrict__ keys, const int *__restrict__ idx,
                                                                         const int *__restrict__ head, const int *__restrict__ vox,
                                                                         unsigned long long *__restrict__ out_keys, int64_t *__restrict__ out_acc,
                                                                         int32_t *__restrict__ out_stamps, int64_t out_capacity, long long *__restrict__ rays)
{
    double T[16];
    pcacc_pose_seed(T, pose);
    int64_t runs = vox[m];
    if (runs > m) runs = m;
    const int lane = lane_id();
    const int64_t m_pad = (m + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; i < m_pad; i += (int64_t)gridDim.x * ACCM_BLOCK) {
        int r = -1;
        long long c = 0, mv = 0, qx = 0, qy = 0, qz = 0, ry = 0;
        int t0 = INT32_MAX, t1 = INT32_MIN;
        if (i < m) {
            const unsigned long long key = keys[i];
            const int h = head[i];
            const int64_t row = accum_point_index(idx[i], m);
            if (key != ACC_INVALID_KEY && row >= 0) {
                const int64_t run = accum_run_index(vox[i], h, runs);
                unsigned long long k2;
                int64_t term[ACC_FIELDS], count;
                if (run >= 0 && accg_row(acc, capacity, m, row, T, out_voxel_size, &k2, term, &count) && k2 == key) {
                    r = (int)run;
                    c = term[0]; mv = term[1]; qx = term[2]; qy = term[3]; qz = term[4];
                    t0 = stamps[row]; t1 = stamps[capacity + row];
                    ry = pierced ? pierced[row] : 0;
                    if (h) out_keys[run] = key;
                }
            }
        }
        c = acc_seg_scan(c, r, lane); mv = acc_seg_scan(mv, r, lane);
        qx = acc_seg_scan(qx, r, lane); qy = acc_seg_scan(qy, r, lane); qz = acc_seg_scan(qz, r, lane);
        if (pierced) ry = acc_seg_scan(ry, r, lane);                             // wave-uniform
        t0 = accg_seg_min(t0, r, lane); t1 = accg_seg_max(t1, r, lane);
        const int r_next = __shfl_down(r, 1, 64);
        if (r >= 0 && (lane == 63 || r_next != r)) {                             // last lane of its run in this wave
            atomicAdd((unsigned long long *)&out_acc[accum_field(0, r, out_capacity)], (unsigned long long)c);
            if (mv) atomicAdd((unsigned long long *)&out_acc[accum_field(1, r, out_capacity)], (unsigned long long)mv);
            atomicAdd((unsigned long long *)&out_acc[accum_field(2, r, out_capacity)], (unsigned long long)qx);
            atomicAdd((unsigned long long *)&out_acc[accum_field(3, r, out_capacity)], (unsigned long long)qy);
            atomicAdd((unsigned long long *)&out_acc[accum_field(4, r, out_capacity)], (unsigned long long)qz);
            if (ry) atomicAdd((unsigned long long *)&rays[r], (unsigned long long)ry);
            atomicMin(&out_stamps[r], t0);
            atomicMax(&out_stamps[out_capacity + r], t1);
        }
    }
}

// G6.  runs_ptr = NULL: an empty map.
static __global__ __launch_bounds__(ACCM_BLOCK) void accg_finish_kernel(const int *__restrict__ runs_ptr, int64_t m, const long long *__restrict__ rays,
                                                                         int32_t *__restrict__ out_pierced, int64_t *counters, int64_t *state,
                                                                         int64_t carry_dropped)
{
    int64_t runs = runs_ptr ? *runs_ptr : 0;
    if (runs > m) runs = m;
    long long saturated = 0;
    if (out_pierced)
        for (int64_t e = (int64_t)blockIdx.x * ACCM_BLOCK + threadIdx.x; e < runs; e += (int64_t)gridDim.x * ACCM_BLOCK) {
            int sat;
            out_pierced[e] = accm_pierced(rays[e], &sat);
            saturated += sat;
        }
    accum_wave_count((unsigned long long *)counters, PCACC_REGRID_SATURATED, saturated);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counters[PCACC_REGRID_ROWS_IN] = m;
        counters[PCACC_REGRID_ROWS_OUT] = runs;
        for (int k = 0; k < PCACC_ACCUM_STATE_WORDS; ++k) state[k] = 0;
        state[PCACC_ACCUM_NUM_VOXELS] = runs;
        state[PCACC_ACCUM_DROPPED] = carry_dropped + counters[PCACC_REGRID_DROPPED_POINTS];     // the key pass has ended: stream order
    }
}

struct AccgWs {
    unsigned long long *key_a, *key_b;
    long long *rays;
    int *idx_a, *idx_b, *head, *vox, *chunk;
    void *sort_tmp;
    size_t sort_tmp_bytes, total;
};

static int accg_carve(int64_t n, char *base, AccgWs *w)
{
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
        return PCACC_E_LAUNCH;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    const size_t un = (size_t)n;
    w->key_a = (unsigned long long *)take(un * 8);
    w->key_b = (unsigned long long *)take(un * 8);
    w->rays = (long long *)take(un * 8);
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

extern "C" int pcacc_accum_regrid_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AccgWs w;
    const int rc = accg_carve(m > 0 ? m : 1, nullptr, &w);
    if (rc != PCACC_OK) return rc;
    *bytes = w.total;
    return PCACC_OK;
}

extern "C" int pcacc_accum_regrid(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced, int64_t in_capacity,
                                  int64_t m, const double *pose, double out_voxel_size, int64_t carry_dropped, int64_t *out_keys, int64_t *out_acc,
                                  int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    if (m < 0 || in_capacity < m || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < m || out_capacity > ACCUM_MAX_CAPACITY || !counters || !state)
        return PCACC_E_ARG;
    if (!(out_voxel_size > 0.0) || !(out_voxel_size - out_voxel_size == 0.0)) return PCACC_E_ARG;
    if (m > 0 && (!in_keys || !in_acc || !in_stamps || !out_keys || !out_acc || !out_stamps || (in_pierced && !out_pierced) || !workspace)) return PCACC_E_ARG;
    if (accum_tables_overlap(in_keys, in_acc, in_stamps, in_pierced, in_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity)) return PCACC_E_ARG;
    AccgWs w;
    if (m > 0) {
        const int rc = accg_carve(m, (char *)workspace, &w);
        if (rc != PCACC_OK) return rc;
        if (workspace_bytes < w.total) return PCACC_E_WORKSPACE;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, PCACC_REGRID_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) {
        hipLaunchKernelGGL(accg_finish_kernel, dim3(1), dim3(ACCM_BLOCK), 0, st, (const int *)nullptr, m, (const long long *)nullptr, (int32_t *)nullptr,
                           counters, state, carry_dropped);
        PCACC_CHECK_LAUNCH();
        return PCACC_OK;
    }
    const int grid = pcacc_grid(m, ACCM_BLOCK);
    int32_t *op = in_pierced ? out_pierced : (int32_t *)nullptr;
    hipLaunchKernelGGL(accg_keys_kernel, dim3(grid), dim3(ACCM_BLOCK), 0, st, in_acc, in_capacity, m, pose, out_voxel_size, w.key_a, w.idx_a,
                       (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    if (rocprim::radix_sort_pairs(w.sort_tmp, w.sort_tmp_bytes, w.key_a, w.key_b, w.idx_a, w.idx_b, (size_t)m, 0, 64, st) != hipSuccess)
        return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(accg_heads_kernel, dim3(grid), dim3(ACCM_BLOCK), 0, st, (const unsigned long long *)w.key_b, m, w.head);
    pcacc_scan_i32(w.head, m, w.chunk, w.vox, st);                                                // vox[m] = rows of the new map
    hipLaunchKernelGGL(accg_clear_kernel, dim3(grid), dim3(ACCM_BLOCK), 0, st, (const int *)(w.vox + m), m, out_acc, out_stamps, out_capacity, w.rays);
    hipLaunchKernelGGL(accg_reduce_kernel, dim3(grid), dim3(ACCM_BLOCK), 0, st, in_acc, in_stamps, in_pierced, in_capacity, m, pose, out_voxel_size,
                       (const unsigned long long *)w.key_b, (const int *)w.idx_b, (const int *)w.head, (const int *)w.vox, (unsigned long long *)out_keys,
                       out_acc, out_stamps, out_capacity, w.rays);
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accg_finish_kernel, dim3(grid), dim3(ACCM_BLOCK), 0, st, (const int *)(w.vox + m), m, (const long long *)w.rays, op, counters, state,
                       carry_dropped);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
