// C4. Accumulated scene cloud: a persistent voxel map that takes one window of points per call (include/pcacc.h C4).
//
// The map is SORTED: `keys` ascending and duplicate-free, the integer records field-major beside it.  No hash table, no floating-point
// atomics; every record field is an integer, so the map depends neither on the order of the points inside a call nor on the run.
//   add      K1 keys        key (or the all-ones invalid key, which sorts to the end) and row number of every point; dropped points counted
//            K2 rocPRIM     radix sort of (key, row) on 64 bits
//            K3 heads+scan  run heads of the sorted keys -> number of the window voxel of every sorted position, U window voxels (scan.h)
//            K4 reduce      per-point contributions (recomputed from the row with the arithmetic of K1) summed per run: a segmented scan over
//                           the 64 lanes of a wave, then ONE 64-bit integer atomic per (wave, run) and field -- a wall of 5000 points in one
//                           voxel costs 79 atomics per field, not 5000, and integer additions commute
//            K5 search      every window voxel binary-searched in the map: hit or miss, and its insertion position; misses scanned
//            K6 decide      one thread: M + misses against the capacity of the output tables -> status; NOTHING has touched a table so far
//            K7 merge       old entry p -> p + (misses below it), its record plus the window's when the window holds its key;
//                           missed window voxel j -> position + rank.  Out of place: the input tables stay as they were.
//   extract  keep flags -> scan -> compaction in key order.
// Every table index goes through a helper of accum_grid.h, which the host build bounds-checks.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "scan.h"
#include "accum_launch.h"

#define ACC_BLOCK 256
#define ACC_MAX_POINTS ((int64_t)1 << 30)         // int scans and int row numbers
static_assert(ACC_BLOCK == ACCUM_KEEP_BLOCK, "extract launches accum_keep_kernel on its own grid");

struct AccHdr {                                     // device words of one call, zeroed first
    unsigned long long dropped;                     // invalid points of this call
    long long m;                                    // voxels of the input map
    long long total;                                // m + misses
    int go;                                         // 1: the merge may write
    int bad;                                        // 1: the state word did not fit the input tables
};

struct AccPose { double t[12]; };

static __device__ __forceinline__ AccPose acc_load_pose(const double *pose)
{
    AccPose p;
#pragma unroll
    for (int k = 0; k < 12; ++k) p.t[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);     // NULL = identity, through the same arithmetic
    return p;
}

// K1.  A thread takes 4 consecutive points: three 16-byte loads when the table is 16-byte aligned.
static __global__ __launch_bounds__(ACC_BLOCK) void accum_keys_kernel(const float *__restrict__ points, int64_t n, const double *__restrict__ pose,
                                                                       double voxel_size, int aligned, unsigned long long *__restrict__ key_out,
                                                                       int *__restrict__ idx_out, AccHdr *hdr)
{
    const AccPose T = acc_load_pose(pose);
    const int64_t groups = (n + 3) >> 2;
    int dropped = 0;
    for (int64_t g = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; g < groups; g += (int64_t)gridDim.x * ACC_BLOCK) {
        const int64_t i0 = g * 4;
        float v[12];
        if (aligned && i0 + 4 <= n) {
            const float4 *src = reinterpret_cast<const float4 *>(points) + g * 3;
            const float4 a = src[0], b = src[1], c = src[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = (i0 * 3 + k < n * 3) ? points[i0 * 3 + k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            unsigned long long key;
            int64_t q[3];
            if (!accum_point(T.t, v + 3 * j, voxel_size, &key, q)) { key = ACC_INVALID_KEY; ++dropped; }
            key_out[i] = key;
            idx_out[i] = (int)i;
        }
    }
    __shared__ int lds[4];
    int tot;
    block256_exclusive_scan(dropped, lds, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&hdr->dropped, (unsigned long long)tot);
}

// K3.
static __global__ __launch_bounds__(ACC_BLOCK) void accum_heads_kernel(const unsigned long long *__restrict__ keys, int64_t n, int *__restrict__ head)
{
    for (int64_t i = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACC_BLOCK) {
        const unsigned long long k = keys[i];
        head[i] = (k != ACC_INVALID_KEY && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
    }
}

// window tables [ACC_FIELDS][n]: rows below the number of window voxels cleared
static __global__ __launch_bounds__(ACC_BLOCK) void accum_zero_kernel(long long *__restrict__ wacc, const int *__restrict__ runs_ptr, int64_t n)
{
    const int64_t runs = *runs_ptr;
    for (int64_t e = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; e < runs * ACC_FIELDS; e += (int64_t)gridDim.x * ACC_BLOCK) {
        const int f = (int)(e / runs);
        wacc[accum_field(f, e - f * runs, n)] = 0;
    }
}

// K4.  A wave takes 64 consecutive sorted positions per pass; all 64 lanes stay in the loop (the bound is wave-uniform).
static __global__ __launch_bounds__(ACC_BLOCK) void accum_reduce_kernel(const float *__restrict__ points, int64_t n, const double *__restrict__ pose,
                                                                         const uint8_t *__restrict__ moving, double voxel_size,
                                                                         const unsigned long long *__restrict__ keys, const int *__restrict__ idx,
                                                                         const int *__restrict__ head, const int *__restrict__ vox,
                                                                         unsigned long long *__restrict__ wkey, long long *__restrict__ wacc)
{
    const AccPose T = acc_load_pose(pose);
    const int64_t runs = vox[n];
    const int lane = lane_id();
    const int64_t n_pad = (n + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * ACC_BLOCK) {
        int r = -1;
        long long c = 0, mv = 0, qx = 0, qy = 0, qz = 0;
        if (i < n) {
            const unsigned long long key = keys[i];
            const int h = head[i];
            const int64_t row = accum_point_index(idx[i], n);
            if (key != ACC_INVALID_KEY && row >= 0) {
                const int64_t run = accum_run_index(vox[i], h, runs);
                unsigned long long k2;
                int64_t q[3];
                const float p[3] = {points[3 * row], points[3 * row + 1], points[3 * row + 2]};
                if (run >= 0 && accum_point(T.t, p, voxel_size, &k2, q) && k2 == key) {
                    r = (int)run;
                    c = 1; mv = (moving && moving[row]) ? 1 : 0; qx = q[0]; qy = q[1]; qz = q[2];
                    if (h) wkey[run] = key;
                }
            }
        }
        c = acc_seg_scan(c, r, lane); mv = acc_seg_scan(mv, r, lane);
        qx = acc_seg_scan(qx, r, lane); qy = acc_seg_scan(qy, r, lane); qz = acc_seg_scan(qz, r, lane);
        const int r_next = __shfl_down(r, 1, 64);
        if (r >= 0 && (lane == 63 || r_next != r)) {             // last lane of its run in this wave
            atomicAdd((unsigned long long *)&wacc[accum_field(0, r, n)], (unsigned long long)c);
            if (mv) atomicAdd((unsigned long long *)&wacc[accum_field(1, r, n)], (unsigned long long)mv);
            atomicAdd((unsigned long long *)&wacc[accum_field(2, r, n)], (unsigned long long)qx);
            atomicAdd((unsigned long long *)&wacc[accum_field(3, r, n)], (unsigned long long)qy);
            atomicAdd((unsigned long long *)&wacc[accum_field(4, r, n)], (unsigned long long)qz);
        }
    }
}

// the state word against the input tables, before anything reads them
static __global__ void accum_begin_kernel(const int64_t *state, int64_t in_capacity, AccHdr *hdr)
{
    const long long m = state[PCACC_ACCUM_NUM_VOXELS];
    if (m < 0 || m > in_capacity) { hdr->bad = 1; hdr->m = 0; }
    else hdr->m = m;
}

// K5.  miss[j] = 0 for j past the window's voxels, so that the scan may run over n entries (n is what the host knows).
static __global__ __launch_bounds__(ACC_BLOCK) void accum_search_kernel(const unsigned long long *__restrict__ wkey, const int *__restrict__ runs_ptr, int64_t n,
                                                                         const unsigned long long *__restrict__ map_keys, const AccHdr *hdr,
                                                                         int *__restrict__ miss, int *__restrict__ pos)
{
    const int64_t runs = *runs_ptr, m = hdr->m;
    for (int64_t j = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * ACC_BLOCK) {
        int ms = 0, ps = 0;
        if (j < runs) {
            const unsigned long long key = wkey[j];
            const int64_t p = accum_lower_bound(map_keys, m, key);
            ms = !(p < m && map_keys[p] == key);
            ps = (int)p;
        }
        miss[j] = ms;
        pos[j] = ps;
    }
}

// K6.
static __global__ void accum_decide_kernel(int64_t *state, AccHdr *hdr, const int *vox, const int *mrank, int64_t n, int64_t out_capacity)
{
    const long long total = hdr->m + mrank[n];
    hdr->total = total;
    state[PCACC_ACCUM_NEEDED] = total;
    state[PCACC_ACCUM_WINDOW_VOXELS] = vox[n];
    state[PCACC_ACCUM_WINDOW_DROPPED] = (int64_t)hdr->dropped;
    if (hdr->bad) { state[PCACC_ACCUM_STATUS] = PCACC_ACCUM_BAD_STATE; hdr->go = 0; }
    else if (total > out_capacity) { state[PCACC_ACCUM_STATUS] = PCACC_ACCUM_TOO_SMALL; hdr->go = 0; }
    else {
        state[PCACC_ACCUM_STATUS] = PCACC_ACCUM_OK;
        state[PCACC_ACCUM_NUM_VOXELS] = total;
        state[PCACC_ACCUM_DROPPED] += (int64_t)hdr->dropped;
        hdr->go = 1;
    }
}

// K7a.  Old entries.
static __global__ __launch_bounds__(ACC_BLOCK) void accum_merge_old_kernel(const unsigned long long *__restrict__ in_keys, const long long *__restrict__ in_acc,
                                                                            const int32_t *__restrict__ in_stamps, int64_t in_capacity,
                                                                            const unsigned long long *__restrict__ wkey, const long long *__restrict__ wacc,
                                                                            const int *__restrict__ runs_ptr, const int *__restrict__ mrank, int64_t n, int32_t stamp,
                                                                            unsigned long long *__restrict__ out_keys, long long *__restrict__ out_acc,
                                                                            int32_t *__restrict__ out_stamps, int64_t out_capacity, const AccHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t m = hdr->m, total = hdr->total, runs = *runs_ptr;
    for (int64_t p = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; p < m; p += (int64_t)gridDim.x * ACC_BLOCK) {
        const unsigned long long key = in_keys[p];
        const int64_t j = accum_lower_bound(wkey, runs, key);              // in [0, runs]; mrank has n + 1 >= runs + 1 entries
        const int64_t d = accum_merge_dst(p, mrank[j], total);
        if (d < 0) continue;
        const bool hit = j < runs && wkey[j] == key;
        out_keys[d] = key;
#pragma unroll
        for (int f = 0; f < ACC_FIELDS; ++f)
            out_acc[accum_field(f, d, out_capacity)] = in_acc[accum_field(f, p, in_capacity)] + (hit ? wacc[accum_field(f, j, n)] : 0);
        const int32_t t0 = in_stamps[p], t1 = in_stamps[in_capacity + p];
        out_stamps[d] = (hit && stamp < t0) ? stamp : t0;
        out_stamps[out_capacity + d] = (hit && stamp > t1) ? stamp : t1;
    }
}

// K7b.  Window voxels the map did not hold.
static __global__ __launch_bounds__(ACC_BLOCK) void accum_merge_new_kernel(const unsigned long long *__restrict__ wkey, const long long *__restrict__ wacc,
                                                                            const int *__restrict__ runs_ptr, const int *__restrict__ miss, const int *__restrict__ pos,
                                                                            const int *__restrict__ mrank, int64_t n, int32_t stamp,
                                                                            unsigned long long *__restrict__ out_keys, long long *__restrict__ out_acc,
                                                                            int32_t *__restrict__ out_stamps, int64_t out_capacity, const AccHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total, runs = *runs_ptr;
    for (int64_t j = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; j < runs; j += (int64_t)gridDim.x * ACC_BLOCK) {
        if (!miss[j]) continue;
        const int64_t d = accum_merge_dst(pos[j], mrank[j], total);
        if (d < 0) continue;
        out_keys[d] = wkey[j];
#pragma unroll
        for (int f = 0; f < ACC_FIELDS; ++f) out_acc[accum_field(f, d, out_capacity)] = wacc[accum_field(f, j, n)];
        out_stamps[d] = stamp;
        out_stamps[out_capacity + d] = stamp;
    }
}

struct AccWs {
    AccHdr *hdr;
    unsigned long long *key_a, *key_b, *wkey;
    long long *wacc;
    int *idx_a, *idx_b, *head, *vox, *miss, *pos, *mrank, *chunk;
    void *sort_tmp;
    size_t sort_tmp_bytes, total;
};

static int acc_ws_layout(int64_t n, char *base, AccWs *w)
{
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
        return PCACC_E_LAUNCH;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    const size_t un = (size_t)n;
    w->hdr = (AccHdr *)take(sizeof(AccHdr));
    w->key_a = (unsigned long long *)take(un * 8);
    w->key_b = (unsigned long long *)take(un * 8);
    w->wkey = (unsigned long long *)take(un * 8);
    w->wacc = (long long *)take(un * 8 * ACC_FIELDS);
    w->idx_a = (int *)take(un * 4);
    w->idx_b = (int *)take(un * 4);
    w->head = (int *)take(un * 4);
    w->vox = (int *)take((un + 1) * 4);
    w->miss = (int *)take(un * 4);
    w->pos = (int *)take(un * 4);
    w->mrank = (int *)take((un + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(n) * 4);
    w->sort_tmp = take(sort_bytes);
    w->sort_tmp_bytes = sort_bytes;
    w->total = off;
    return PCACC_OK;
}

extern "C" int pcacc_accum_add_workspace_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > ACC_MAX_POINTS) return PCACC_E_ARG;
    AccWs w;
    const int rc = acc_ws_layout(n > 0 ? n : 1, nullptr, &w);
    if (rc != PCACC_OK) return rc;
    *bytes = w.total;
    return PCACC_OK;
}

extern "C" int pcacc_accum_add(const float *points, int64_t n, const double *pose, const uint8_t *moving, int32_t stamp, double voxel_size,
                               const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, int64_t in_capacity,
                               int64_t *out_keys, int64_t *out_acc, int32_t *out_stamps, int64_t out_capacity,
                               int64_t *state, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 1 || n > ACC_MAX_POINTS || !points || !state || !workspace) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    if (in_capacity < 0 || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < 1 || out_capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (in_capacity > 0 && (!in_keys || !in_acc || !in_stamps)) return PCACC_E_ARG;
    if (!out_keys || !out_acc || !out_stamps) return PCACC_E_ARG;
    if (out_keys == in_keys || out_acc == in_acc || out_stamps == in_stamps) return PCACC_E_ARG;     // the merge is out of place
    AccWs w;
    const int rc = acc_ws_layout(n, (char *)workspace, &w);
    if (rc != PCACC_OK) return rc;
    if (workspace_bytes < w.total) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    const int grid = pcacc_grid(n, ACC_BLOCK);

    if (hipMemsetAsync(w.hdr, 0, sizeof(AccHdr), st) != hipSuccess) return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(accum_begin_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)state, in_capacity, w.hdr);
    hipLaunchKernelGGL(accum_keys_kernel, dim3(pcacc_grid((n + 3) / 4, ACC_BLOCK)), dim3(ACC_BLOCK), 0, st, points, n, pose, voxel_size,
                       (int)(((uintptr_t)points & 15) == 0), w.key_a, w.idx_a, w.hdr);
    PCACC_CHECK_LAUNCH();
    if (rocprim::radix_sort_pairs(w.sort_tmp, w.sort_tmp_bytes, w.key_a, w.key_b, w.idx_a, w.idx_b, (size_t)n, 0, 64, st) != hipSuccess)
        return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(accum_heads_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, (const unsigned long long *)w.key_b, n, w.head);
    pcacc_scan_i32(w.head, n, w.chunk, w.vox, st);                                                  // vox[n] = window voxels
    hipLaunchKernelGGL(accum_zero_kernel, dim3(pcacc_grid(n * ACC_FIELDS, ACC_BLOCK)), dim3(ACC_BLOCK), 0, st, w.wacc, (const int *)(w.vox + n), n);
    hipLaunchKernelGGL(accum_reduce_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, points, n, pose, moving, voxel_size,
                       (const unsigned long long *)w.key_b, (const int *)w.idx_b, (const int *)w.head, (const int *)w.vox, w.wkey, w.wacc);
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accum_search_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, (const unsigned long long *)w.wkey, (const int *)(w.vox + n), n,
                       (const unsigned long long *)in_keys, (const AccHdr *)w.hdr, w.miss, w.pos);
    pcacc_scan_i32(w.miss, n, w.chunk, w.mrank, st);                                                // mrank[n] = misses
    hipLaunchKernelGGL(accum_decide_kernel, dim3(1), dim3(1), 0, st, state, w.hdr, (const int *)w.vox, (const int *)w.mrank, n, out_capacity);
    PCACC_CHECK_LAUNCH();
    if (in_capacity > 0)
        hipLaunchKernelGGL(accum_merge_old_kernel, dim3(pcacc_grid(in_capacity, ACC_BLOCK)), dim3(ACC_BLOCK), 0, st, (const unsigned long long *)in_keys,
                           (const long long *)in_acc, in_stamps, in_capacity, (const unsigned long long *)w.wkey, (const long long *)w.wacc,
                           (const int *)(w.vox + n), (const int *)w.mrank, n, stamp, (unsigned long long *)out_keys, (long long *)out_acc, out_stamps,
                           out_capacity, (const AccHdr *)w.hdr);
    hipLaunchKernelGGL(accum_merge_new_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, (const unsigned long long *)w.wkey, (const long long *)w.wacc,
                       (const int *)(w.vox + n), (const int *)w.miss, (const int *)w.pos, (const int *)w.mrank, n, stamp, (unsigned long long *)out_keys,
                       (long long *)out_acc, out_stamps, out_capacity, (const AccHdr *)w.hdr);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// ---- extract ---------------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(ACC_BLOCK) void accum_compact_kernel(const unsigned long long *__restrict__ keys, const long long *__restrict__ acc,
                                                                          const int32_t *__restrict__ stamps, int64_t capacity, int64_t m,
                                                                          const int *__restrict__ keep, const int *__restrict__ kpos,
                                                                          float *__restrict__ out_points, int32_t *__restrict__ out_coords,
                                                                          int64_t *__restrict__ out_count, int64_t *__restrict__ out_moving,
                                                                          int32_t *__restrict__ out_t_first, int32_t *__restrict__ out_t_last, int64_t *out_n)
{
    const int64_t kept = kpos[m];
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_n = kept;
    for (int64_t i = (int64_t)blockIdx.x * ACC_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACC_BLOCK) {
        if (!keep[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, kept);                // in [0, kept), kept <= m = rows of every output
        if (d < 0) continue;
        const long long count = acc[accum_field(0, i, capacity)];
        int32_t c[3];
        accum_unkey(keys[i], c);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out_points[3 * d + a] = accum_centroid(acc[accum_field(2 + a, i, capacity)], count);
            out_coords[3 * d + a] = c[a];
        }
        out_count[d] = count;
        out_moving[d] = acc[accum_field(1, i, capacity)];
        out_t_first[d] = stamps[i];
        out_t_last[d] = stamps[capacity + i];
    }
}

static size_t acc_extract_ws(int64_t m, int **keep, int **kpos, int **chunk, char *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    *keep = (int *)take((size_t)m * 4);
    *kpos = (int *)take((size_t)(m + 1) * 4);
    *chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    return off;
}

extern "C" int pcacc_accum_extract_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    int *a, *b, *c;
    *bytes = acc_extract_ws(m > 0 ? m : 1, &a, &b, &c, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_extract(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                                   int32_t use_fraction, double max_moving_fraction, float *out_points, int32_t *out_coords, int64_t *out_count,
                                   int64_t *out_moving, int32_t *out_t_first, int32_t *out_t_last, int64_t *out_n,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || !out_n) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (m == 0) return hipMemsetAsync(out_n, 0, sizeof(int64_t), st) == hipSuccess ? PCACC_OK : PCACC_E_LAUNCH;
    if (!keys || !acc || !stamps || !out_points || !out_coords || !out_count || !out_moving || !out_t_first || !out_t_last || !workspace) return PCACC_E_ARG;
    int *keep, *kpos, *chunk;
    if (workspace_bytes < acc_extract_ws(m, &keep, &kpos, &chunk, (char *)workspace)) return PCACC_E_WORKSPACE;
    const int grid = pcacc_grid(m, ACC_BLOCK);
    hipLaunchKernelGGL(accum_keep_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, acc, capacity, m, min_count, (int)use_fraction,
                       max_moving_fraction, keep);
    pcacc_scan_i32(keep, m, chunk, kpos, st);
    hipLaunchKernelGGL(accum_compact_kernel, dim3(grid), dim3(ACC_BLOCK), 0, st, (const unsigned long long *)keys, (const long long *)acc, stamps, capacity, m,
                       (const int *)keep, (const int *)kpos, out_points, out_coords, out_count, out_moving, out_t_first, out_t_last, out_n);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
