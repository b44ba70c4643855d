// C11. Connected components of the accumulated scene cloud and the removal of the small ones, on the device (include/pcacc.h C11).
//
//   rows      pass 1 of C5 (accn_rows_launch): dst[m], extract's row of every map row, -1 = filtered out; rows[kept] its inverse; kept stays on the device.
//   init      parent[j] = j over extract rows.
//   link      one lane per extract row in a grid-stride loop, consecutive lanes on consecutive rows: accc_edges of accum_components.h -- the code the
//             host build runs with every index assert-checked -- and one join per edge (union_find.h: the larger root under the smaller by atomicCAS,
//             relaxed agent-scope loads, paths halved; a join gives up after ACCC_UNION_TRIES lost attempts and sets GAVE_UP).  The three row counts
//             are summed per lane, reduced over the wave, one integer atomic per wave and non-zero counter.
//   flatten   parent[j] = root of j.  The walk stores nothing on its way (uf_root): a slot is written by its own lane only, so no halving store of a
//             neighbour can land behind the lane's own and leave the slot under an inner node.
//   number    root flags (takes part and parent[j] == j) -> scan.h -> component number: a root is the smallest row of its set, so the scan numbers the
//             components in ascending order of their smallest key with no sort.  The lane of row j writes label[j]; the lane of a root also writes
//             first_row and the neutral elements of its component's record.
//   stats     one lane per extract row: its row's contribution (accc_stat_row), an inclusive segmented scan over runs of equal label among
//             consecutive lanes (accc_stat_merge), and the last lane of a run adds the run's total to the component: one 64-bit atomicAdd or 32-bit
//             atomicMin / atomicMax per (wave, run) and field, not one per voxel -- a ground component of two million voxels is a run of 64 in
//             almost every wave.  Integers only: the tables do not depend on the order.
//   finish    one lane per component: voxels, the centroid (accc_centroid), and the largest component by a wave maximum and one atomicMax per wave.
//   removal   flag (accc_row_small) -> scan -> compaction through accr_move_row / accum_merge_dst, as accum_prune.hip; one lane per component counts
//             the components that went and stayed.
// A mask that does not fit the kept count is found by every kernel itself (BAD_MASK): nothing is read back.  No floating-point atomics, no LDS beyond
// the scan's, no inline assembly.
#include "scan.h"
#include "accum_components.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCC_BLOCK 256

static_assert(ACCC_COUNTERS == PCACC_COMPONENTS_COUNTERS && ACCC_C_ROWS == PCACC_COMPONENTS_ROWS && ACCC_C_PARTICIPATING == PCACC_COMPONENTS_PARTICIPATING &&
              ACCC_C_OUTSIDE == PCACC_COMPONENTS_OUTSIDE && ACCC_C_MASKED == PCACC_COMPONENTS_MASKED && ACCC_C_COMPONENTS == PCACC_COMPONENTS_K &&
              ACCC_C_LARGEST == PCACC_COMPONENTS_LARGEST && ACCC_C_STATUS == PCACC_COMPONENTS_STATUS && ACCC_OK == PCACC_COMPONENTS_OK &&
              ACCC_BAD_MASK == PCACC_COMPONENTS_BAD_MASK && ACCC_GAVE_UP == PCACC_COMPONENTS_GAVE_UP &&
              ACCC_REMOVE_COUNTERS == PCACC_COMPONENTS_REMOVE_COUNTERS && ACCC_R_KEPT == PCACC_COMPONENTS_REMOVE_KEPT &&
              ACCC_R_SMALL == PCACC_COMPONENTS_REMOVE_SMALL && ACCC_R_COMPONENTS_REMOVED == PCACC_COMPONENTS_REMOVED &&
              ACCC_R_COMPONENTS_KEPT == PCACC_COMPONENTS_SURVIVED, "accum_components.h and include/pcacc.h name the same counters and codes");

struct AcccMap {                         // named scalars: nothing here is indexed at run time
    const unsigned long long *keys;
    const int64_t *acc;
    const int32_t *stamps;
    const uint8_t *mask;
    const int *dst, *rows;
    const int64_t *kept;
    int64_t capacity, m, mask_rows;
    int radius;
};

struct AcccOut {
    int32_t *label, *voxels;
    int64_t *points, *moving, *sum_q;
    float *centroid;
    int32_t *lo, *hi, *t_first, *t_last, *first_row;
    unsigned long long *counters;
};

static __device__ __forceinline__ int64_t accc_kept(const AcccMap &M)
{
    const int64_t kept = *M.kept;
    return kept > M.m ? M.m : (kept < 0 ? 0 : kept);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_init_kernel(int64_t m, int *__restrict__ parent)
{
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < m; j += (int64_t)gridDim.x * ACCC_BLOCK) parent[j] = (int)j;
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_link_kernel(AcccMap M, int *__restrict__ parent, unsigned long long *__restrict__ counters)
{
    const int64_t kept = accc_kept(M);
    const bool fits = accc_mask_fits(M.mask, M.mask_rows, kept);                             // uniform over the grid
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                               // the memset left 0; no lane adds to these
        counters[ACCC_C_ROWS] = (unsigned long long)M.m;
        counters[ACCC_C_OUTSIDE] = (unsigned long long)(M.m - kept);
        if (!fits) {
            counters[ACCC_C_MASKED] = (unsigned long long)kept;
            counters[ACCC_C_STATUS] = ACCC_BAD_MASK;
        }
    }
    if (!fits) return;
    long long c_part = 0, c_masked = 0;
    bool gave_up = false;
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int64_t i = M.rows[j];
        if (i < 0 || i >= M.m || M.dst[i] != j) continue;                                    // a table that does not fit addresses nothing
        if (!accc_takes_part(M.mask, kept, j)) { c_masked += 1; continue; }
        c_part += 1;
        accc_edges(M.keys, M.m, M.dst, M.mask, kept, i, j, M.radius, [&](int64_t a, int64_t b) {
            if (uf_union_bounded(parent, (int)a, (int)b, ACCC_UNION_TRIES) < 0) gave_up = true;
        });
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACCC_C_PARTICIPATING, c_part);
    accum_wave_count(counters, ACCC_C_MASKED, c_masked);
    if (gave_up) atomicMax(&counters[ACCC_C_STATUS], (unsigned long long)ACCC_GAVE_UP);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_flatten_kernel(AcccMap M, int *__restrict__ parent)
{
    const int64_t kept = accc_kept(M);
    if (!accc_mask_fits(M.mask, M.mask_rows, kept)) return;
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int r = uf_root(parent, (int)j);
        if (r != (int)j) uf_store(&parent[j], r);
    }
}

// flag[j] = extract row j is the root of a component; 0 for every slot behind kept (the scan runs over m slots).
static __global__ __launch_bounds__(ACCC_BLOCK) void accc_root_kernel(AcccMap M, const int *__restrict__ parent, int *__restrict__ flag)
{
    const int64_t kept = accc_kept(M);
    const bool fits = accc_mask_fits(M.mask, M.mask_rows, kept);
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < M.m; j += (int64_t)gridDim.x * ACCC_BLOCK)
        flag[j] = (fits && j < kept && accc_takes_part(M.mask, kept, j) && parent[j] == (int)j) ? 1 : 0;
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_label_kernel(AcccMap M, const int *__restrict__ parent, const int *__restrict__ cid, AcccOut out,
                                                                        unsigned long long *__restrict__ vox64)
{
    const int64_t kept = accc_kept(M);
    const bool fits = accc_mask_fits(M.mask, M.mask_rows, kept);
    const int64_t n_comp = cid[M.m];
    if (blockIdx.x == 0 && threadIdx.x == 0) out.counters[ACCC_C_COMPONENTS] = (unsigned long long)n_comp;
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACCC_BLOCK) {
        int32_t lab = -1;
        if (fits && accc_takes_part(M.mask, kept, j)) {
            const int64_t root = accn_index(parent[j], kept);
            const int64_t c = root < 0 ? -1 : accn_index(cid[root], n_comp);
            lab = (int32_t)c;
            if (c >= 0 && root == j) {                                                       // the root's lane: the neutral record of component c
                out.first_row[c] = (int32_t)j;
                vox64[c] = 0; out.points[c] = 0; out.moving[c] = 0;
                out.sum_q[3 * c] = 0; out.sum_q[3 * c + 1] = 0; out.sum_q[3 * c + 2] = 0;
                out.lo[3 * c] = ACCC_I32_MAX; out.lo[3 * c + 1] = ACCC_I32_MAX; out.lo[3 * c + 2] = ACCC_I32_MAX;
                out.hi[3 * c] = ACCC_I32_MIN; out.hi[3 * c + 1] = ACCC_I32_MIN; out.hi[3 * c + 2] = ACCC_I32_MIN;
                out.t_first[c] = ACCC_I32_MAX; out.t_last[c] = ACCC_I32_MIN;
            }
        }
        out.label[j] = lab;
    }
}

static __device__ __forceinline__ void accc_stat_from_lane(AcccStat *o, const AcccStat &s, int d)
{
    o->voxels = __shfl_up((long long)s.voxels, d, 64); o->points = __shfl_up((long long)s.points, d, 64); o->moving = __shfl_up((long long)s.moving, d, 64);
    o->sq_x = __shfl_up((long long)s.sq_x, d, 64); o->sq_y = __shfl_up((long long)s.sq_y, d, 64); o->sq_z = __shfl_up((long long)s.sq_z, d, 64);
    o->lo_x = __shfl_up(s.lo_x, d, 64); o->lo_y = __shfl_up(s.lo_y, d, 64); o->lo_z = __shfl_up(s.lo_z, d, 64);
    o->hi_x = __shfl_up(s.hi_x, d, 64); o->hi_y = __shfl_up(s.hi_y, d, 64); o->hi_z = __shfl_up(s.hi_z, d, 64);
    o->t_first = __shfl_up(s.t_first, d, 64); o->t_last = __shfl_up(s.t_last, d, 64);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_stats_kernel(AcccMap M, AcccOut out, unsigned long long *__restrict__ vox64)
{
    const int64_t kept = accc_kept(M);
    if (!accc_mask_fits(M.mask, M.mask_rows, kept)) return;
    const int64_t n_comp = (int64_t)out.counters[ACCC_C_COMPONENTS];                         // written by the launch before this one
    const int lane = lane_id();
    for (int64_t base = (int64_t)blockIdx.x * ACCC_BLOCK; base < kept; base += (int64_t)gridDim.x * ACCC_BLOCK) {      // uniform: all 64 lanes shuffle
        const int64_t j = base + threadIdx.x;
        int lab = -1;
        AcccStat s;
        accc_stat_none(&s);
        if (j < kept) {
            const int64_t i = M.rows[j];
            const int l = out.label[j];
            if (l >= 0 && l < n_comp && i >= 0 && i < M.m && M.dst[i] == j && accc_stat_row(M.keys, M.acc, M.stamps, M.capacity, M.m, i, &s)) lab = l;
        }
        // runs of equal label among consecutive lanes: the run's first lane, then an inclusive scan that never crosses it
        const int before = __shfl_up(lab, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || before != lab);
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            AcccStat o;
            accc_stat_from_lane(&o, s, d);
            if (lane - d >= start) accc_stat_merge(&s, o);
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0;
        if (tail && lab >= 0) {
            const int64_t c = lab;
            atomicAdd(&vox64[c], (unsigned long long)s.voxels);
            atomicAdd((unsigned long long *)&out.points[c], (unsigned long long)s.points);
            atomicAdd((unsigned long long *)&out.moving[c], (unsigned long long)s.moving);
            atomicAdd((unsigned long long *)&out.sum_q[3 * c], (unsigned long long)s.sq_x);
            atomicAdd((unsigned long long *)&out.sum_q[3 * c + 1], (unsigned long long)s.sq_y);
            atomicAdd((unsigned long long *)&out.sum_q[3 * c + 2], (unsigned long long)s.sq_z);
            atomicMin(&out.lo[3 * c], s.lo_x); atomicMin(&out.lo[3 * c + 1], s.lo_y); atomicMin(&out.lo[3 * c + 2], s.lo_z);
            atomicMax(&out.hi[3 * c], s.hi_x); atomicMax(&out.hi[3 * c + 1], s.hi_y); atomicMax(&out.hi[3 * c + 2], s.hi_z);
            atomicMin(&out.t_first[c], s.t_first);
            atomicMax(&out.t_last[c], s.t_last);
        }
    }
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_finish_kernel(int64_t m, AcccOut out, const unsigned long long *__restrict__ vox64)
{
    int64_t n_comp = (int64_t)out.counters[ACCC_C_COMPONENTS];
    if (n_comp > m) n_comp = m;
    long long largest = 0;
    for (int64_t c = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; c < n_comp; c += (int64_t)gridDim.x * ACCC_BLOCK) {
        const long long v = (long long)vox64[c];
        const int64_t points = out.points[c];
        out.voxels[c] = (int32_t)v;
        out.centroid[3 * c] = points > 0 ? accc_centroid(out.sum_q[3 * c], points) : 0.f;
        out.centroid[3 * c + 1] = points > 0 ? accc_centroid(out.sum_q[3 * c + 1], points) : 0.f;
        out.centroid[3 * c + 2] = points > 0 ? accc_centroid(out.sum_q[3 * c + 2], points) : 0.f;
        largest = v > largest ? v : largest;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(largest, d, 64);
        largest = o > largest ? o : largest;
    }
    if (lane_id() == 0 && largest > 0) atomicMax(&out.counters[ACCC_C_LARGEST], (unsigned long long)largest);
}

// ---- removal ------------------------------------------------------------------------------------------------------------------------------------------
struct AcccRemove {
    const int *dst;
    const int64_t *kept, *first;         // first: the counters of pcacc_accum_components
    const int32_t *label, *voxels;
    const int64_t *points;
    int64_t m, min_voxels, min_points;
    int dry_run;
};

static __device__ __forceinline__ bool accc_first_ok(const AcccRemove &R) { return R.first[ACCC_C_STATUS] == ACCC_OK; }

static __device__ __forceinline__ int64_t accc_first_components(const AcccRemove &R)
{
    const int64_t k = R.first[ACCC_C_COMPONENTS];
    return k > R.m ? R.m : (k < 0 ? 0 : k);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_small_kernel(AcccRemove R, int *__restrict__ flag)
{
    int64_t kept = *R.kept;
    if (kept > R.m) kept = R.m;
    const bool ok = accc_first_ok(R);
    const int64_t n_comp = accc_first_components(R);
    for (int64_t i = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; i < R.m; i += (int64_t)gridDim.x * ACCC_BLOCK)
        flag[i] = (ok && accc_row_small(R.dst, R.label, R.voxels, R.points, kept, n_comp, i, R.m, R.min_voxels, R.min_points)) ? 0 : 1;
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_compact_kernel(const unsigned long long *__restrict__ in_keys, const int64_t *__restrict__ in_acc,
                                                                          const int32_t *__restrict__ in_stamps, const int32_t *__restrict__ in_pierced,
                                                                          int64_t in_capacity, AcccRemove R, const int *__restrict__ flag,
                                                                          const int *__restrict__ kpos, unsigned long long *__restrict__ out_keys,
                                                                          int64_t *__restrict__ out_acc, int32_t *__restrict__ out_stamps,
                                                                          int32_t *__restrict__ out_pierced, int64_t out_capacity,
                                                                          unsigned long long *__restrict__ counters, int64_t *__restrict__ state)
{
    const int64_t kept = kpos[R.m];
    const bool dry = R.dry_run != 0 || !accc_first_ok(R);
    long long c_kept = 0, c_small = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; i < R.m; i += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int keep = flag[i];
        c_kept += keep != 0; c_small += keep == 0;
        if (dry || !keep) continue;
        accr_move_row(in_keys, in_acc, in_stamps, in_pierced, in_capacity, R.m, i, out_keys, out_acc, out_stamps, out_pierced, out_capacity, kept,
                      accum_merge_dst(kpos[i], 0, kept));
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACCC_R_KEPT, c_kept);
    accum_wave_count(counters, ACCC_R_SMALL, c_small);
    if (!dry && blockIdx.x == 0 && threadIdx.x == 0) state[PCACC_ACCUM_NUM_VOXELS] = kept;
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_component_count_kernel(AcccRemove R, unsigned long long *__restrict__ counters)
{
    const bool ok = accc_first_ok(R);
    const int64_t n_comp = accc_first_components(R);
    long long c_removed = 0, c_kept = 0;
    for (int64_t c = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; c < n_comp; c += (int64_t)gridDim.x * ACCC_BLOCK) {
        const bool small = ok && accc_small(R.voxels[c], R.points[c], R.min_voxels, R.min_points);
        c_removed += small; c_kept += !small;
    }
    accum_wave_count(counters, ACCC_R_COMPONENTS_REMOVED, c_removed);
    accum_wave_count(counters, ACCC_R_COMPONENTS_KEPT, c_kept);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------
struct AcccWs : AccnRowsWs { int *parent, *flag, *cid, *chunk; unsigned long long *vox64; };

static size_t accc_carve(AcccWs *w, char *base, int64_t m)                                   // m >= 1
{
    size_t off = accn_rows_ws_carve(m, w, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->parent = (int *)take((size_t)m * 4);
    w->flag = (int *)take((size_t)m * 4);
    w->cid = (int *)take((size_t)(m + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    w->vox64 = (unsigned long long *)take((size_t)m * 8);
    return off;
}

extern "C" int pcacc_accum_components_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AcccWs w;
    *bytes = accc_carve(&w, nullptr, m > 0 ? m : 1);
    return PCACC_OK;
}

extern "C" int pcacc_accum_components(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                                      int32_t use_fraction, double max_moving_fraction, const uint8_t *mask, int64_t mask_rows, int32_t radius,
                                      int32_t *out_label, int32_t *out_voxels, int64_t *out_points, int64_t *out_moving, int64_t *out_sum_q,
                                      float *out_centroid, int32_t *out_lo, int32_t *out_hi, int32_t *out_t_first, int32_t *out_t_last,
                                      int32_t *out_first_row, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || radius < 1 || radius > ACCN_MAX_RADIUS || mask_rows < 0 || !counters) return PCACC_E_ARG;
    AcccWs w;
    if (m > 0) {
        if (!keys || !acc || !stamps || !workspace || (mask_rows > 0 && !mask)) return PCACC_E_ARG;
        if (!out_label || !out_voxels || !out_points || !out_moving || !out_sum_q || !out_centroid || !out_lo || !out_hi || !out_t_first || !out_t_last ||
            !out_first_row)
            return PCACC_E_ARG;
        if (workspace_bytes < accc_carve(&w, (char *)workspace, m)) return PCACC_E_ARG;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCC_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return PCACC_OK;
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    AcccMap M;
    M.keys = (const unsigned long long *)keys; M.acc = acc; M.stamps = stamps; M.mask = mask; M.dst = w.rows.dst; M.rows = w.rows.rows; M.kept = w.kept;
    M.capacity = capacity; M.m = m; M.mask_rows = mask_rows; M.radius = (int)radius;
    const AcccOut out = {out_label, out_voxels, out_points, out_moving, out_sum_q, out_centroid, out_lo, out_hi, out_t_first, out_t_last, out_first_row,
                         (unsigned long long *)counters};
    const int grid = pcacc_grid(m, ACCC_BLOCK);
    hipLaunchKernelGGL(accc_init_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, m, w.parent);
    // a lane runs up to (2r+1)^2 serial searches: many small workgroups spread over the CUs, as accum_normals.hip
    hipLaunchKernelGGL(accc_link_kernel, dim3(pcacc_grid(m, ACCC_BLOCK, 1 << 22)), dim3(ACCC_BLOCK), 0, st, M, w.parent, (unsigned long long *)counters);
    hipLaunchKernelGGL(accc_flatten_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, w.parent);
    hipLaunchKernelGGL(accc_root_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, (const int *)w.parent, w.flag);
    PCACC_CHECK_LAUNCH();
    pcacc_scan_i32(w.flag, m, w.chunk, w.cid, st);                                                // cid[m] = K
    hipLaunchKernelGGL(accc_label_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, (const int *)w.parent, (const int *)w.cid, out, w.vox64);
    hipLaunchKernelGGL(accc_stats_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, out, w.vox64);
    hipLaunchKernelGGL(accc_finish_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, m, out, (const unsigned long long *)w.vox64);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

extern "C" int pcacc_accum_remove_components(const int64_t *in_keys, const int64_t *in_acc, const int32_t *in_stamps, const int32_t *in_pierced,
                                             int64_t in_capacity, int64_t m, int64_t min_count, int32_t use_fraction, double max_moving_fraction,
                                             const int32_t *label, const int32_t *voxels, const int64_t *points, const int64_t *components_counters,
                                             int64_t min_voxels, int64_t min_points, int32_t dry_run, int64_t *out_keys, int64_t *out_acc,
                                             int32_t *out_stamps, int32_t *out_pierced, int64_t out_capacity, int64_t *counters, int64_t *state,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || in_capacity < m || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < m || out_capacity > ACCUM_MAX_CAPACITY || !counters) return PCACC_E_ARG;
    if (min_voxels < 0 || min_points < 0) return PCACC_E_ARG;
    if (accum_tables_overlap(in_keys, in_acc, in_stamps, in_pierced, in_capacity, out_keys, out_acc, out_stamps, out_pierced, out_capacity)) return PCACC_E_ARG;
    AcccWs w;
    if (m > 0) {
        if (!in_keys || !in_acc || !in_stamps || !workspace || !label || !voxels || !points || !components_counters) return PCACC_E_ARG;
        if (!dry_run && (!out_keys || !out_acc || !out_stamps || !state || (in_pierced && !out_pierced))) return PCACC_E_ARG;
        if (workspace_bytes < accc_carve(&w, (char *)workspace, m)) return PCACC_E_ARG;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCC_REMOVE_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return PCACC_OK;
    if (accn_rows_launch(in_acc, in_capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    AcccRemove R;
    R.dst = w.rows.dst; R.kept = w.kept; R.first = components_counters; R.label = label; R.voxels = voxels; R.points = points;
    R.m = m; R.min_voxels = min_voxels; R.min_points = min_points; R.dry_run = dry_run != 0 ? 1 : 0;
    const int grid = pcacc_grid(m, ACCC_BLOCK);
    hipLaunchKernelGGL(accc_small_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, R, w.flag);
    pcacc_scan_i32(w.flag, m, w.chunk, w.cid, st);                                                // cid[m] = rows kept
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accc_compact_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, (const unsigned long long *)in_keys, in_acc, in_stamps, in_pierced,
                       in_capacity, R, (const int *)w.flag, (const int *)w.cid, (unsigned long long *)out_keys, out_acc, out_stamps,
                       in_pierced ? out_pierced : (int32_t *)nullptr, out_capacity, (unsigned long long *)counters, state);
    hipLaunchKernelGGL(accc_component_count_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, R, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
