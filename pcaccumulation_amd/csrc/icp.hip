// C3. Point-to-point ICP of J independent (source segment, target segment) jobs -- the test-time pose refinement of models/egomotion.py:9-28,
// :360-384 (model.ego_icp) and models/alignnet.py:54-112 (model.tpointnet_icp), which the reference runs through Open3D's registration_icp on
// the host, one call per frame and per instance.  include/pcacc.h (C3) has the contract; DESIGN.md section 9b the argument.
//
//   icp_setup    validates the segment and job tables (a bad table stops every later kernel: nothing is addressed through it), marks the target
//                segments, seeds every job's pose with its initial pose.
//   icp_insert   every finite, in-range point of a target segment claims the hash slot of its (segment, cell) key with one 64-bit CAS and
//                counts itself there; icp_fill (behind a scan of the counts: scan.h) writes the point lists.  The index is built ONCE per call:
//                the target of a job is fixed over all rounds, and the T - 1 jobs of a sample share one target segment.
//   icp_corr     round r, workgroup (job, slice): every lane runs icp_lane_sums of icp_round.h -- the slice's source points under the job's current
//                pose, nearest target through the 27-cell walk of icp_grid.h, 17 float64 sums (count, sum q, sum t, sum t q^T, sum d^2) -- and the
//                workgroup reduces them in icp_tree_sum's order in LDS into the slot of (job, slice).
//   icp_update   round r, one wave per job: the slots added in slice order, then icp_round of icp_round.h on one lane: fitness / rmse, the
//                convergence test against the previous round, the least-squares rigid update (Umeyama without scale on svd3.h's SVD) composed
//                onto the pose.
// Every value a result depends on is computed by icp_grid.h / icp_round.h, the code the host build runs with every index assert-checked; this file
// holds the index build, the LDS tree and the launches.  All arithmetic on coordinates is float64.  No floating-point atomics, no order that depends
// on scheduling: the order of the entries in a cell's list does (integer atomics), but the walk picks by (distance^2, index), so two runs give the
// same bits, and they are the host build's.  Convergence is per job on the device; a finished job's later rounds return at once; the host never
// waits inside the loop (2 * (max_iter + 1) launches, queued back to back).
#include "common.h"
#include "icp_round.h"
#include "scan.h"

#define ICP_BAD_TABLE 1            // ctrl[0]

struct IcpWs {
    unsigned long long *keys;      // [slots]      | zero-filled per call
    int32_t *cnt;                  // [slots]      | counts, then (cleared by the scan) the fill cursors
    int32_t *tflag;                // [n_seg]      | 1 = some job's target
    int32_t *ctrl;                 // [16]         | [0] ICP_BAD_TABLE
    size_t zero_bytes;
    int32_t *start;                // [slots + 1]
    int32_t *pslot;                // [n] slot of a stored target point, -1 otherwise
    int32_t *list;                 // [n]
    int32_t *sums;                 // [chunks of slots + 1]
    double *partial;               // [J][slices][ICP_SUMS]
    IcpState *state;               // [J]
    uint32_t slots;
    int slices;
};

static bool icp_sizes_ok(int64_t n, int32_t n_seg, int32_t n_jobs, int32_t max_iter)
{
    return n >= 0 && n <= (1ll << 29) && n_seg >= 1 && n_seg <= ICP_MAX_SEGMENTS && n_jobs >= 0 && n_jobs <= (1 << 20) && max_iter >= 0 &&
           max_iter <= 10000;
}

static size_t icp_carve(IcpWs *w, char *base, int64_t n, int32_t n_seg, int32_t n_jobs)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += pcacc_align(bytes); return p; };
    uint32_t slots = 64;
    while ((int64_t)slots < 2 * n) slots <<= 1;
    w->slots = slots;
    w->slices = icp_slices(n, n_jobs);
    w->keys = (unsigned long long *)take((size_t)slots * 8);
    w->cnt = (int32_t *)take((size_t)slots * 4);
    w->tflag = (int32_t *)take((size_t)n_seg * 4);
    w->ctrl = (int32_t *)take(16 * 4);
    w->zero_bytes = off;
    w->start = (int32_t *)take(((size_t)slots + 1) * 4);
    w->pslot = (int32_t *)take((size_t)(n > 0 ? n : 1) * 4);
    w->list = (int32_t *)take((size_t)(n > 0 ? n : 1) * 4);
    w->sums = (int32_t *)take(((size_t)pcacc_chunks(slots) + 1) * 4);
    w->partial = (double *)take((size_t)(n_jobs > 0 ? n_jobs : 1) * w->slices * ICP_SUMS * 8);
    w->state = (IcpState *)take((size_t)(n_jobs > 0 ? n_jobs : 1) * sizeof(IcpState));
    return off;
}

extern "C" int pcacc_icp_point_to_point_workspace_bytes(int64_t n, int32_t n_seg, int32_t n_jobs, size_t *bytes)
{
    if (!bytes || !icp_sizes_ok(n, n_seg, n_jobs, 0)) return PCACC_E_ARG;
    IcpWs w;
    *bytes = icp_carve(&w, nullptr, n, n_seg, n_jobs);
    return 0;
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_setup(const int32_t *__restrict__ offsets, int n_seg, const int32_t *__restrict__ jobs, int n_jobs,
                                                       int64_t n, const double *__restrict__ init, IcpWs w)
{
    const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i <= n_seg) {
        const int64_t a = offsets[i];
        bool bad = a < 0 || a > n;
        if (i < n_seg && a > (int64_t)offsets[i + 1]) bad = true;
        if (bad) atomicOr(&w.ctrl[0], ICP_BAD_TABLE);
    }
    if (i < n_jobs) {
        const int src = jobs[2 * i], tgt = jobs[2 * i + 1];
        IcpState &s = w.state[i];
        if (src < 0 || src >= n_seg || tgt < 0 || tgt >= n_seg) atomicOr(&w.ctrl[0], ICP_BAD_TABLE);
        else w.tflag[tgt] = 1;
        pcacc_pose_seed(s.T, init ? init + 16 * (int64_t)i : nullptr);
        s.fit = s.rmse = 0.0;
        s.done = s.iters = s.status = s.pad = 0;
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_insert(const float *__restrict__ points, int64_t n, const int32_t *__restrict__ offsets, int n_seg,
                                                        double h, IcpWs w)
{
    if (w.ctrl[0] != 0) return;
    const uint32_t mask = w.slots - 1;
    for (int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ICP_BLOCK) {
        int slot = -1;
        const int seg = icp_segment_of(offsets, n_seg, i);
        if (seg >= 0 && w.tflag[seg]) {
            const double p[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
            int c[3];
            if (icp_target_cell(p, h, c)) {
                const unsigned long long key = icp_key(seg, c[0], c[1], c[2]);
                uint32_t s = icp_hash(key, mask);
                for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {     // slots >= 2 n: an empty slot always exists
                    const unsigned long long k = atomicCAS(&w.keys[s], 0ull, key);
                    if (k == 0 || k == key) { slot = (int)s; break; }
                }
                if (slot >= 0) atomicAdd(&w.cnt[slot], 1);
            }
        }
        w.pslot[i] = slot;
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_fill(int64_t n, IcpWs w)
{
    if (w.ctrl[0] != 0) return;
    for (int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ICP_BLOCK) {
        const int s = w.pslot[i];
        if (s < 0) continue;
        const int64_t e = (int64_t)w.start[s] + atomicAdd(&w.cnt[s], 1);
        if (e >= 0 && e < n) w.list[e] = (int32_t)i;                        // e < start[s + 1] <= stored points <= n by construction
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_corr(const float *__restrict__ points, int64_t n, const int32_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ jobs, double h, double thr2, IcpWs w)
{
    __shared__ double red[ICP_SUMS][ICP_BLOCK];
    const int j = blockIdx.x, slice = blockIdx.y;
    if (w.ctrl[0] != 0 || w.state[j].done) return;                          // uniform over the workgroup
    const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
    int64_t a, b;
    icp_slice_bounds(offsets[src], offsets[src + 1], w.slices, slice, &a, &b);
    IcpGrid g;
    g.keys = w.keys; g.start = w.start; g.list = w.list; g.points = points; g.mask = w.slots - 1; g.n = n; g.n_list = n; g.h = h;
    double T[12], acc[ICP_SUMS];
    for (int k = 0; k < 12; ++k) T[k] = w.state[j].T[k];
    icp_lane_sums(g, tgt, T, thr2, a, b, threadIdx.x, acc);
    for (int k = 0; k < ICP_SUMS; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = ICP_BLOCK / 2; s > 0; s >>= 1) {                           // icp_tree_sum's order
        if ((int)threadIdx.x < s)
            for (int k = 0; k < ICP_SUMS; ++k) red[k][threadIdx.x] = red[k][threadIdx.x] + red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < ICP_SUMS) w.partial[((int64_t)j * w.slices + slice) * ICP_SUMS + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void icp_update(const int32_t *__restrict__ offsets, const int32_t *__restrict__ jobs, int round, int max_iter,
                                                 IcpWs w, double *__restrict__ out_T, double *__restrict__ out_fit, double *__restrict__ out_rmse,
                                                 int32_t *__restrict__ out_iters, int32_t *__restrict__ out_status)
{
#pragma clang fp contract(off)
    __shared__ double sums[ICP_SUMS];
    const int j = blockIdx.x;
    IcpState &st = w.state[j];
    if (w.ctrl[0] != 0) {                                                   // a table that cannot be trusted: identity, and the status says so
        if (threadIdx.x == 0 && round == 0) {
            pcacc_pose_seed(out_T + 16 * (int64_t)j, nullptr);
            out_fit[j] = out_rmse[j] = 0.0;
            out_iters[j] = 0;
            out_status[j] = PCACC_ICP_BAD_TABLE;
        }
        return;
    }
    if (st.done) return;
    if (threadIdx.x < ICP_SUMS) {
        double v = 0.0;
        for (int s = 0; s < w.slices; ++s) v += w.partial[((int64_t)j * w.slices + s) * ICP_SUMS + threadIdx.x];     // slice order
        sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
    const IcpOut o = {out_T + 16 * (int64_t)j, out_fit + j, out_rmse + j, out_iters + j, out_status + j};
    icp_round(&st, sums, (int64_t)offsets[src + 1] - offsets[src], (int64_t)offsets[tgt + 1] - offsets[tgt], round, max_iter, &o);
}

extern "C" int pcacc_icp_point_to_point(const float *points, int64_t n, const int32_t *seg_offsets, int32_t n_seg, const int32_t *jobs,
                                        int32_t n_jobs, const double *init, double threshold, int32_t max_iter, double *out_T,
                                        double *out_fitness, double *out_rmse, int32_t *out_iters, int32_t *out_status, void *ws, size_t ws_bytes,
                                        void *stream)
{
    if (!icp_sizes_ok(n, n_seg, n_jobs, max_iter) || !seg_offsets || !ws) return PCACC_E_ARG;
    if (!(threshold > 0.0) || !(threshold < 1e300)) return PCACC_E_ARG;
    if (n > 0 && !points) return PCACC_E_ARG;
    if (n_jobs == 0) return 0;
    if (!jobs || !out_T || !out_fitness || !out_rmse || !out_iters || !out_status) return PCACC_E_ARG;
    IcpWs w;
    const size_t need = icp_carve(&w, (char *)ws, n, n_seg, n_jobs);
    if (ws_bytes < need) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(ws, 0, w.zero_bytes, st) != hipSuccess) return PCACC_E_LAUNCH;
    const int setup_items = n_jobs > n_seg + 1 ? n_jobs : n_seg + 1;
    hipLaunchKernelGGL(icp_setup, dim3((setup_items + ICP_BLOCK - 1) / ICP_BLOCK), dim3(ICP_BLOCK), 0, st, seg_offsets, n_seg, jobs, n_jobs, n, init, w);
    if (n > 0) hipLaunchKernelGGL(icp_insert, dim3(pcacc_grid(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, points, n, seg_offsets, n_seg, threshold, w);
    pcacc_scan_i32(w.cnt, (int64_t)w.slots, w.sums, w.start, st, w.cnt);                    // the histogram becomes the cursor array of the fill pass
    if (n > 0) hipLaunchKernelGGL(icp_fill, dim3(pcacc_grid(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, n, w);
    PCACC_CHECK_LAUNCH();
    const double thr2 = threshold * threshold;
    for (int round = 0; round <= max_iter; ++round) {
        hipLaunchKernelGGL(icp_corr, dim3(n_jobs, w.slices), dim3(ICP_BLOCK), 0, st, points, n, seg_offsets, jobs, threshold, thr2, w);
        hipLaunchKernelGGL(icp_update, dim3(n_jobs), dim3(64), 0, st, seg_offsets, jobs, round, max_iter, w, out_T, out_fitness, out_rmse,
                           out_iters, out_status);
    }
    PCACC_CHECK_LAUNCH();
    return 0;
}
