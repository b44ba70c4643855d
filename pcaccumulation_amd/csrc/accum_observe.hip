// C14. Observed space: a second sorted voxel table that records which voxels measured rays crossed (include/pcacc.h C14).
//
// The route of accum.hip with a walk in front of it; every piece of index arithmetic is a function of accum_observe.h, which the host build checks.
//   observe  K0 begin       the state words against the input table
//            K1 count       one lane per ray: acco_walk with a visit that only counts; the five counters reduced per wave as C7 does
//            scan           visit counts -> offsets and the total V (scan.h)
//            K2 decide      one thread: V against visit_capacity -> TOO_MANY, or the emit may run
//            K3 emit        the same walk again, every ray writes its keys at its offset; the list is padded to visit_capacity with the invalid key
//            rocPRIM        radix sort of the keys on 64 bits (the invalid key sorts to the end)
//            K4 heads+scan  run heads of the sorted keys; the length of a run is the ray count of a voxel in this call -- no atomics
//            K5 runs        key and first position of every run
//            K6 search+scan every run binary-searched in the table: hit or miss, and its insertion position; misses scanned
//            K7 decide      one thread: m + misses against the capacity of the output tables -> status; NOTHING has touched a table so far
//            K8 merge       old row p -> p + (misses below it), the run added where there is one; missed run j -> position + rank.  Out of place.
//   lookup   one launch, one lane per row: acco_lookup.
// The host knows n and visit_capacity, the device alone knows V: every pass over the visits runs its grid over visit_capacity and stops at V.
#include <rocprim/device/device_radix_sort.hpp>

#include "scan.h"
#include "accum_observe.h"
#include "accum_launch.h"

#define ACCO_BLOCK 256
#define ACCO_MAX_POINTS ((int64_t)1 << 30)
#define ACCO_MAX_VISIT_CAPACITY (((int64_t)1 << 31) - 1)

static_assert(ACCO_OK == PCACC_ACCUM_OK && ACCO_TOO_SMALL == PCACC_ACCUM_TOO_SMALL && ACCO_BAD_STATE == PCACC_ACCUM_BAD_STATE &&
              ACCO_TOO_MANY == PCACC_OBSERVE_TOO_MANY, "accum_observe.h restates the status values of include/pcacc.h");
static_assert(ACCO_VALID == PCACC_OBSERVED_VALID && ACCO_SEEN == PCACC_OBSERVED_SEEN && ACCO_ENOUGH == PCACC_OBSERVED_ENOUGH,
              "accum_observe.h restates the lookup bits of include/pcacc.h");
static_assert(PCACC_OBSERVE_DROPPED == PCACC_OBSERVE_WALKED + 1 && PCACC_OBSERVE_SKIPPED == PCACC_OBSERVE_WALKED + 2 &&
              PCACC_OBSERVE_TRUNCATED == PCACC_OBSERVE_WALKED + 3 && PCACC_OBSERVE_VISITS == PCACC_OBSERVE_WALKED + 4, "the five counters are consecutive");

struct AccoHdr {                                    // device words of one call, zeroed first
    unsigned long long counters[5];                 // walked, dropped, skipped, truncated, visits of this call
    long long m;                                    // rows of the input table
    long long V;                                    // visits the emit writes: 0 unless emit is 1
    long long total;                                // m + misses
    int emit;                                       // 1: V fits, the walk may write its keys
    int go;                                         // 1: the merge may write
    int bad;                                        // 1: the state words did not fit the input table
};

struct AccoRays {                                   // the scan and origin arguments, as pcacc_accum_pierce takes them
    const float *points;
    int64_t n;
    const uint8_t *moving;
    const double *origins;
    int64_t n_origins;
    const int32_t *origin_index;
    const double *pose;
    double voxel_size, margin, max_range;
    int use_range, max_steps;
};

// One ray through acco_walk.  The origin is copied into registers before the call: a select between two pointers would send the walk through scratch memory.
template <class Visit>
static __device__ __forceinline__ AccoWalk acco_one_ray(const AccoRays &a, const double *T, int64_t i, Visit &visit)
{
    const float p[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
    const int64_t row = accp_origin_index(a.origin_index ? (int64_t)a.origin_index[i] : 0, a.n_origins);
    double o[3] = {0.0, 0.0, 0.0};
    if (row >= 0) { o[0] = a.origins[3 * row]; o[1] = a.origins[3 * row + 1]; o[2] = a.origins[3 * row + 2]; }
    return acco_walk(T, p, o, row >= 0, a.moving && a.moving[i], a.voxel_size, a.margin, a.use_range != 0, a.max_range, a.max_steps, visit);
}

// K0.
static __global__ void acco_begin_kernel(const int64_t *state, int64_t in_capacity, AccoHdr *hdr)
{
    const long long m = state[PCACC_OBSERVE_NUM_VOXELS];
    if (m < 0 || m > in_capacity) { hdr->bad = 1; hdr->m = 0; }
    else hdr->m = m;
}

// K1.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_count_kernel(AccoRays a, int *__restrict__ count, AccoHdr *hdr)
{
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = a.pose ? a.pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);    // NULL = identity, through the same arithmetic
    long long c_walked = 0, c_dropped = 0, c_skipped = 0, c_truncated = 0, c_visits = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * ACCO_BLOCK) {
        AccoCount visit;
        const AccoWalk r = acco_one_ray(a, T, i, visit);
        count[i] = r.visits;
        c_walked += r.status == ACCP_WALKED; c_dropped += r.status == ACCP_DROPPED; c_skipped += r.status == ACCP_SKIPPED;
        c_truncated += r.truncated; c_visits += r.visits;
    }
    // every lane of the wave arrives here: one atomic per wave and counter
    accum_wave_count(hdr->counters, 0, c_walked);
    accum_wave_count(hdr->counters, 1, c_dropped);
    accum_wave_count(hdr->counters, 2, c_skipped);
    accum_wave_count(hdr->counters, 3, c_truncated);
    accum_wave_count(hdr->counters, 4, c_visits);
}

// K2.  offsets[n] = V.
static __global__ void acco_decide_visits_kernel(int64_t *state, AccoHdr *hdr, const int *offsets, int64_t n, int64_t visit_capacity)
{
    const long long V = offsets[n];
    const int status = acco_decide_visits(hdr->bad != 0, V, visit_capacity);
    state[PCACC_OBSERVE_CALL_VISITS] = V;
    if (status == ACCO_OK) { hdr->emit = 1; hdr->V = V; return; }
    hdr->emit = 0; hdr->V = 0;
    state[PCACC_OBSERVE_STATUS] = status;
    if (status == ACCO_TOO_MANY) state[PCACC_OBSERVE_NEEDED_VISITS] = V;
}

// K3.  The walk of K1 again; then the slots behind V take the invalid key, so that the sort has visit_capacity defined keys.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_emit_kernel(AccoRays a, const int *__restrict__ offsets, unsigned long long *__restrict__ key_out,
                                                                       int64_t visit_capacity, const AccoHdr *hdr)
{
    const int64_t V = hdr->V;
    if (hdr->emit) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = a.pose ? a.pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
        for (int64_t i = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * ACCO_BLOCK) {
            AccoEmit visit = {key_out, 0, 0};
            if (!acco_slots(offsets, i, a.n, V, &visit.at, &visit.end) || visit.at == visit.end) continue;
            acco_one_ray(a, T, i, visit);
        }
    }
    for (int64_t i = V + (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < visit_capacity; i += (int64_t)gridDim.x * ACCO_BLOCK) key_out[i] = ACC_INVALID_KEY;
}

// K4.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_heads_kernel(const unsigned long long *__restrict__ sorted, int64_t visit_capacity, const AccoHdr *hdr,
                                                                        int *__restrict__ head)
{
    const int64_t V = hdr->V;
    for (int64_t i = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < visit_capacity; i += (int64_t)gridDim.x * ACCO_BLOCK) head[i] = acco_head(sorted, i, V);
}

// K5.  run_start has visit_capacity + 1 entries: entry R closes the last run.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_runs_kernel(const unsigned long long *__restrict__ sorted, const int *__restrict__ head,
                                                                       const int *__restrict__ vox, int64_t visit_capacity, const AccoHdr *hdr,
                                                                       unsigned long long *__restrict__ run_key, int *__restrict__ run_start)
{
    const int64_t V = hdr->V, R = vox[visit_capacity];
    if (blockIdx.x == 0 && threadIdx.x == 0 && R >= 0 && R <= visit_capacity) run_start[R] = (int)V;
    for (int64_t i = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < V; i += (int64_t)gridDim.x * ACCO_BLOCK) {
        if (!head[i]) continue;
        const int64_t r = accum_run_index(vox[i], 1, R);
        if (r < 0) continue;
        run_key[r] = sorted[i];
        run_start[r] = (int)i;
    }
}

// K6.  miss[j] = 0 for j past the runs, so that the scan may run over visit_capacity entries (which is what the host knows).
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_search_kernel(const unsigned long long *__restrict__ run_key, const int *__restrict__ runs_ptr,
                                                                         int64_t visit_capacity, const unsigned long long *__restrict__ in_keys, const AccoHdr *hdr,
                                                                         int *__restrict__ miss, int *__restrict__ pos)
{
    const int64_t R = *runs_ptr, m = hdr->m;
    for (int64_t j = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; j < visit_capacity; j += (int64_t)gridDim.x * ACCO_BLOCK) {
        int ms = 0, ps = 0;
        if (j < R) ps = (int)acco_search(in_keys, m, run_key[j], &ms);
        miss[j] = ms;
        pos[j] = ps;
    }
}

// K7.  On any status other than OK the cumulative counters and NUM_VOXELS stay: a retry counts nothing twice.
static __global__ void acco_decide_rows_kernel(int64_t *state, AccoHdr *hdr, const int *vox, const int *mrank, int64_t visit_capacity, int64_t out_capacity)
{
    if (!hdr->emit) { hdr->go = 0; return; }
    const long long total = hdr->m + mrank[visit_capacity];
    hdr->total = total;
    state[PCACC_OBSERVE_NEEDED] = total;
    state[PCACC_OBSERVE_CALL_VOXELS] = vox[visit_capacity];
    const int status = acco_decide_rows(total, out_capacity);
    state[PCACC_OBSERVE_STATUS] = status;
    hdr->go = status == ACCO_OK;
    if (!hdr->go) return;
    state[PCACC_OBSERVE_NUM_VOXELS] = total;
    for (int k = 0; k < 5; ++k) state[PCACC_OBSERVE_WALKED + k] += (int64_t)hdr->counters[k];
}

// K8a.  Old rows.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_merge_old_kernel(const unsigned long long *__restrict__ in_keys, const int64_t *__restrict__ in_rays,
                                                                            const int32_t *__restrict__ in_stamps, int64_t in_capacity,
                                                                            const unsigned long long *__restrict__ run_key, const int *__restrict__ run_start,
                                                                            const int *__restrict__ runs_ptr, const int *__restrict__ mrank, int32_t stamp,
                                                                            unsigned long long *__restrict__ out_keys, int64_t *__restrict__ out_rays,
                                                                            int32_t *__restrict__ out_stamps, int64_t out_capacity, const AccoHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t m = hdr->m, total = hdr->total, R = *runs_ptr;
    for (int64_t p = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; p < m; p += (int64_t)gridDim.x * ACCO_BLOCK)
        acco_merge_old(p, in_keys, in_rays, in_stamps, in_capacity, m, run_key, run_start, R, mrank, total, stamp, out_keys, out_rays, out_stamps, out_capacity);
}

// K8b.  Runs the table did not hold.
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_merge_new_kernel(const unsigned long long *__restrict__ run_key, const int *__restrict__ run_start,
                                                                            const int *__restrict__ runs_ptr, const int *__restrict__ miss, const int *__restrict__ pos,
                                                                            const int *__restrict__ mrank, int32_t stamp, unsigned long long *__restrict__ out_keys,
                                                                            int64_t *__restrict__ out_rays, int32_t *__restrict__ out_stamps, int64_t out_capacity,
                                                                            const AccoHdr *hdr)
{
    if (!hdr->go) return;
    const int64_t total = hdr->total, R = *runs_ptr;
    for (int64_t j = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; j < R; j += (int64_t)gridDim.x * ACCO_BLOCK)
        acco_merge_new(j, run_key, run_start, R, miss, pos, mrank, total, stamp, out_keys, out_rays, out_stamps, out_capacity);
}

struct AccoWs {
    AccoHdr *hdr;
    unsigned long long *key_a, *key_b;              // key_a: the emitted keys, and after the sort the run keys; key_b: the sorted keys
    int *count, *offsets, *head, *vox, *run_start, *miss, *pos, *mrank, *chunk;
    void *sort_tmp;
    size_t sort_tmp_bytes, total;
};

static int acco_ws_layout(int64_t n, int64_t visit_capacity, char *base, AccoWs *w)
{
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (size_t)visit_capacity, 0, 64,
                                 (hipStream_t)0) != hipSuccess)
        return PCACC_E_LAUNCH;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    const size_t un = (size_t)n, uc = (size_t)visit_capacity;
    w->hdr = (AccoHdr *)take(sizeof(AccoHdr));
    w->key_a = (unsigned long long *)take(uc * 8);
    w->key_b = (unsigned long long *)take(uc * 8);
    w->count = (int *)take(un * 4);
    w->offsets = (int *)take((un + 1) * 4);
    w->head = (int *)take(uc * 4);
    w->vox = (int *)take((uc + 1) * 4);
    w->run_start = (int *)take((uc + 1) * 4);
    w->miss = (int *)take(uc * 4);
    w->pos = (int *)take(uc * 4);
    w->mrank = (int *)take((uc + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(n > visit_capacity ? n : visit_capacity) * 4);
    w->sort_tmp = take(sort_bytes);
    w->sort_tmp_bytes = sort_bytes;
    w->total = off;
    return PCACC_OK;
}

static bool acco_sizes_ok(int64_t n, int64_t visit_capacity, int64_t in_m)
{
    return n >= 0 && n <= ACCO_MAX_POINTS && visit_capacity >= 1 && visit_capacity <= ACCO_MAX_VISIT_CAPACITY && in_m >= 0 && in_m <= ACCUM_MAX_CAPACITY;
}

extern "C" int pcacc_accum_observe_workspace_bytes(int64_t n, int64_t visit_capacity, int64_t in_m, size_t *bytes)
{
    if (!bytes || !acco_sizes_ok(n, visit_capacity, in_m)) return PCACC_E_ARG;
    AccoWs w;
    const int rc = acco_ws_layout(n > 0 ? n : 1, visit_capacity, nullptr, &w);
    if (rc != PCACC_OK) return rc;
    *bytes = w.total;
    return PCACC_OK;
}

extern "C" int pcacc_accum_observe(const float *points, int64_t n, const uint8_t *moving, const double *origins, int64_t n_origins,
                                   const int32_t *origin_index, const double *pose, int32_t stamp, double voxel_size, double margin, int32_t use_range,
                                   double max_range, int32_t max_steps, int64_t visit_capacity, const int64_t *in_keys, const int64_t *in_rays,
                                   const int32_t *in_stamps, int64_t in_capacity, int64_t *out_keys, int64_t *out_rays, int32_t *out_stamps,
                                   int64_t out_capacity, int64_t *state, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!acco_sizes_ok(n, visit_capacity, 0) || n_origins < 1 || !state) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    if (!(margin >= 0.0) || !(margin - margin == 0.0)) return PCACC_E_ARG;
    if (use_range && !(max_range >= 0.0)) return PCACC_E_ARG;
    if (max_steps < 1 || max_steps > ACCP_MAX_STEPS || !acco_visits_fit(n, max_steps)) return PCACC_E_ARG;
    if (in_capacity < 0 || in_capacity > ACCUM_MAX_CAPACITY || out_capacity < 1 || out_capacity > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    if (in_capacity > 0 && (!in_keys || !in_rays || !in_stamps)) return PCACC_E_ARG;
    if (!out_keys || !out_rays || !out_stamps) return PCACC_E_ARG;
    const void *in_tab[3] = {in_keys, in_rays, in_stamps}, *out_tab[3] = {out_keys, out_rays, out_stamps};
    for (int a = 0; a < 3; ++a)                                                                       // the merge is out of place
        for (int b = 0; b < 3; ++b)
            if (accum_bytes_overlap(in_tab[a], 8 * (size_t)in_capacity, out_tab[b], 8 * (size_t)out_capacity)) return PCACC_E_ARG;
    if (n == 0) return PCACC_OK;
    if (!points || !origins || !workspace) return PCACC_E_ARG;
    AccoWs w;
    const int rc = acco_ws_layout(n, visit_capacity, (char *)workspace, &w);
    if (rc != PCACC_OK) return rc;
    if (workspace_bytes < w.total) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    const AccoRays rays = {points, n, moving, origins, n_origins, origin_index, pose, voxel_size, margin, max_range, use_range ? 1 : 0, (int)max_steps};
    const int64_t C = visit_capacity;
    // a lane walks hundreds of voxels: many small workgroups spread over the CUs, as accum_pierce.hip
    const dim3 ray_grid(pcacc_grid(n, ACCO_BLOCK, 1 << 22)), visit_grid(pcacc_grid(C, ACCO_BLOCK)), block(ACCO_BLOCK);

    if (hipMemsetAsync(w.hdr, 0, sizeof(AccoHdr), st) != hipSuccess) return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(acco_begin_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)state, in_capacity, w.hdr);
    hipLaunchKernelGGL(acco_count_kernel, ray_grid, block, 0, st, rays, w.count, w.hdr);
    PCACC_CHECK_LAUNCH();
    pcacc_scan_i32(w.count, n, w.chunk, w.offsets, st);                                               // offsets[n] = V
    hipLaunchKernelGGL(acco_decide_visits_kernel, dim3(1), dim3(1), 0, st, state, w.hdr, (const int *)w.offsets, n, C);
    hipLaunchKernelGGL(acco_emit_kernel, ray_grid, block, 0, st, rays, (const int *)w.offsets, w.key_a, C, (const AccoHdr *)w.hdr);
    PCACC_CHECK_LAUNCH();
    if (rocprim::radix_sort_keys(w.sort_tmp, w.sort_tmp_bytes, w.key_a, w.key_b, (size_t)C, 0, 64, st) != hipSuccess) return PCACC_E_LAUNCH;
    hipLaunchKernelGGL(acco_heads_kernel, visit_grid, block, 0, st, (const unsigned long long *)w.key_b, C, (const AccoHdr *)w.hdr, w.head);
    pcacc_scan_i32(w.head, C, w.chunk, w.vox, st);                                                    // vox[C] = R, the voxels of this call
    hipLaunchKernelGGL(acco_runs_kernel, visit_grid, block, 0, st, (const unsigned long long *)w.key_b, (const int *)w.head, (const int *)w.vox, C,
                       (const AccoHdr *)w.hdr, w.key_a, w.run_start);
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(acco_search_kernel, visit_grid, block, 0, st, (const unsigned long long *)w.key_a, (const int *)(w.vox + C), C,
                       (const unsigned long long *)in_keys, (const AccoHdr *)w.hdr, w.miss, w.pos);
    pcacc_scan_i32(w.miss, C, w.chunk, w.mrank, st);                                                  // mrank[C] = misses
    hipLaunchKernelGGL(acco_decide_rows_kernel, dim3(1), dim3(1), 0, st, state, w.hdr, (const int *)w.vox, (const int *)w.mrank, C, out_capacity);
    PCACC_CHECK_LAUNCH();
    if (in_capacity > 0)
        hipLaunchKernelGGL(acco_merge_old_kernel, dim3(pcacc_grid(in_capacity, ACCO_BLOCK)), block, 0, st, (const unsigned long long *)in_keys, in_rays, in_stamps,
                           in_capacity, (const unsigned long long *)w.key_a, (const int *)w.run_start, (const int *)(w.vox + C), (const int *)w.mrank, stamp,
                           (unsigned long long *)out_keys, out_rays, out_stamps, out_capacity, (const AccoHdr *)w.hdr);
    hipLaunchKernelGGL(acco_merge_new_kernel, visit_grid, block, 0, st, (const unsigned long long *)w.key_a, (const int *)w.run_start, (const int *)(w.vox + C),
                       (const int *)w.miss, (const int *)w.pos, (const int *)w.mrank, stamp, (unsigned long long *)out_keys, out_rays, out_stamps, out_capacity,
                       (const AccoHdr *)w.hdr);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

// ---- lookup ----------------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(ACCO_BLOCK) void acco_lookup_kernel(const float *__restrict__ points, const int32_t *__restrict__ coords, int64_t n,
                                                                         const double *__restrict__ pose, double voxel_size,
                                                                         const unsigned long long *__restrict__ keys, const int64_t *__restrict__ rays,
                                                                         const int32_t *__restrict__ stamps, int64_t capacity, int64_t m, int64_t min_rays,
                                                                         int64_t *__restrict__ out_rays, int32_t *__restrict__ out_stamps,
                                                                         uint8_t *__restrict__ out_status, unsigned long long *__restrict__ counters)
{
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    long long c_rows = 0, c_valid = 0, c_seen = 0, c_enough = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCO_BLOCK) {
        unsigned long long key = 0;
        bool valid;
        if (points) {
            const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
            int64_t q[3];
            valid = accum_point(T, p, voxel_size, &key, q);
        } else {
            const int32_t c[3] = {coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]};
            valid = acco_coord_key(c, &key);
        }
        int64_t r;
        int32_t t0, t1;
        const int status = acco_lookup(valid, key, keys, rays, stamps, capacity, m, min_rays, &r, &t0, &t1);
        out_rays[i] = r; out_stamps[i] = t0; out_stamps[n + i] = t1; out_status[i] = (uint8_t)status;
        c_rows += 1; c_valid += (status & ACCO_VALID) != 0; c_seen += (status & ACCO_SEEN) != 0; c_enough += (status & ACCO_ENOUGH) != 0;
    }
    accum_wave_count(counters, PCACC_OBSERVED_ROWS, c_rows);
    accum_wave_count(counters, PCACC_OBSERVED_N_VALID, c_valid);
    accum_wave_count(counters, PCACC_OBSERVED_N_SEEN, c_seen);
    accum_wave_count(counters, PCACC_OBSERVED_N_ENOUGH, c_enough);
}

// No launch of the lookup takes scratch memory today; the pair of entry points keeps the calling convention of the other rows.
extern "C" int pcacc_accum_observed_lookup_workspace_bytes(int64_t n, int64_t m, size_t *bytes)
{
    if (!bytes || n < 0 || n > ACCO_MAX_POINTS || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    *bytes = 0;
    return PCACC_OK;
}

extern "C" int pcacc_accum_observed_lookup(const float *points, const int32_t *coords, int64_t n, const double *pose, double voxel_size, const int64_t *keys,
                                           const int64_t *rays, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_rays, int64_t *out_rays,
                                           int32_t *out_stamps, uint8_t *out_status, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (n < 0 || n > ACCO_MAX_POINTS || m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || !counters) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    if (n > 0 && ((points != nullptr) == (coords != nullptr))) return PCACC_E_ARG;                   // exactly one of the two
    if (n > 0 && (!out_rays || !out_stamps || !out_status)) return PCACC_E_ARG;
    if (m > 0 && (!keys || !rays || !stamps)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, PCACC_OBSERVED_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;   // written, not added to
    if (n == 0) return PCACC_OK;
    hipLaunchKernelGGL(acco_lookup_kernel, dim3(pcacc_grid(n, ACCO_BLOCK)), dim3(ACCO_BLOCK), 0, st, points, coords, n, pose, voxel_size,
                       (const unsigned long long *)keys, rays, stamps, capacity, m, min_rays, out_rays, out_stamps, out_status, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
