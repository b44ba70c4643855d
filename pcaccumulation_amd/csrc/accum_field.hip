// C19. The exact, truncated Euclidean distance field of a box of voxels of the accumulated scene cloud, its planar form and the lookup of points in it
// (include/pcacc.h C19).
//
//   rows     pass 1 of C5 (accn_rows_launch): rows[kept], the kept count stays on the device.
//   sites    the grid of packed values is filled with none (a memset of ones); one lane per kept row writes its row number at its cell (accf_site: keys
//            are unique, and in planar mode only the first kept row of a column inside the z range writes, so every cell has one writer).
//   passes   the windowed min-plus along z (not when planar), y, x, between two grids of the workspace; the last pass cuts at R^2 and unpacks into the
//            two outputs.  Two kernels, both accf_line_min over a different store:
//              line    the axis is contiguous (stride 1: z, or y when planar).  A workgroup takes 256 consecutive cells, stages them and R cells on
//                      either side in LDS (at most 512 values, 4 KiB) and every lane slides over its own line's part of them.
//              direct  the axis is `stride` elements apart: one lane per cell, the window read from global memory (coalesced: neighbouring lanes are
//                      neighbouring inner cells).  An LDS-tiled form of it (128 positions of the axis x 64 inner cells, 64 KiB) was built and measured;
//                      it did not win and is not here (profiles/accum_field_bench.txt).
//   lookup   a separate entry: one launch, one lane per row (accf_lookup).
// The functions named are those of accum_field.h -- the code the host build runs with every index assert-checked.  No atomics but the wave-reduced
// counters (accum_wave_count), nothing read back, the map is read only, no inline assembly.
#include "common.h"
#include "accum_field.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCF_BLOCK ACCF_CHUNK
#define ACCF_MAX_POINTS ((int64_t)1 << 30)

static_assert(ACCF_MAX_RADIUS == PCACC_FIELD_MAX_RADIUS && ACCF_MAX_CELLS == PCACC_FIELD_MAX_CELLS && ACCF_COUNTERS == PCACC_FIELD_COUNTERS &&
              ACCF_C_ROWS == PCACC_FIELD_N_ROWS && ACCF_C_SITES == PCACC_FIELD_N_SITES && ACCF_C_NEAR == PCACC_FIELD_N_NEAR &&
              ACCF_C_FAR == PCACC_FIELD_N_FAR && ACCF_VALID == PCACC_FIELD_VALID && ACCF_INSIDE == PCACC_FIELD_INSIDE && ACCF_NEAR == PCACC_FIELD_NEAR &&
              ACCF_LOOKUP_COUNTERS == PCACC_FIELD_LOOKUP_COUNTERS,
              "accum_field.h and include/pcacc.h name the same limits, counters and bits");
static_assert(ACCF_BLOCK == 256, "the LDS of the line kernel");

typedef unsigned long long u64;

struct AccfOut { int32_t *dist2, *nearest; };

// The store of a pass: the packed value, or (last pass) the cut and the two outputs.  -> 1 when the cell got a result.
template <bool LAST>
static __device__ __forceinline__ int accf_store(u64 v, int64_t e, int R, u64 *__restrict__ out, AccfOut last)
{
    if (!LAST) { out[e] = v; return 0; }
    int32_t d2, row;
    const bool near = accf_cut(v, R, &d2, &row);
    last.dist2[e] = d2;
    last.nearest[e] = row;
    return near ? 1 : 0;
}

static __global__ __launch_bounds__(ACCF_BLOCK) void accf_site_kernel(AcccMap M, const int64_t *__restrict__ kept_ptr, AccfBox box, int64_t cells,
                                                                       u64 *__restrict__ grid, u64 *__restrict__ counters)
{
    const int64_t kept = *kept_ptr;
    M.kept = kept < 0 ? 0 : (kept > M.m ? M.m : kept);
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[ACCF_C_ROWS] = (u64)M.kept;
    long long sites = 0;
    for (int64_t j = (int64_t)blockIdx.x * ACCF_BLOCK + threadIdx.x; j < M.kept; j += (int64_t)gridDim.x * ACCF_BLOCK) {
        const int64_t cell = accf_site(M, box, j);
        if (cell < 0 || cell >= cells) continue;
        grid[cell] = accf_pack(0, j);
        sites += 1;
    }
    accum_wave_count(counters, ACCF_C_SITES, sites);                                            // every lane of the wave arrives here
}

template <bool LAST>
static __global__ __launch_bounds__(ACCF_BLOCK) void accf_direct_kernel(const u64 *__restrict__ in, int64_t cells, int64_t stride, int64_t len, int R,
                                                                         u64 *__restrict__ out, AccfOut last, u64 *__restrict__ counters)
{
    long long near = 0, all = 0;
    for (int64_t e = (int64_t)blockIdx.x * ACCF_BLOCK + threadIdx.x; e < cells; e += (int64_t)gridDim.x * ACCF_BLOCK) {
        near += accf_store<LAST>(accf_pass_cell(in, cells, stride, len, e, R), e, R, out, last);
        all += 1;
    }
    if (LAST) {
        accum_wave_count(counters, ACCF_C_NEAR, near);
        accum_wave_count(counters, ACCF_C_FAR, all - near);
    }
}

// The axis is contiguous: chunks of ACCF_BLOCK cells, each with R cells on either side in LDS.  A chunk may hold several lines, or a part of one.
template <bool LAST>
static __global__ __launch_bounds__(ACCF_BLOCK) void accf_line_kernel(const u64 *__restrict__ in, int64_t cells, int64_t len, int R, u64 *__restrict__ out,
                                                                       AccfOut last, u64 *__restrict__ counters)
{
    __shared__ u64 lds[ACCF_BLOCK + 2 * ACCF_MAX_RADIUS];
    const int64_t chunks = (cells + ACCF_BLOCK - 1) / ACCF_BLOCK;
    long long near = 0, all = 0;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t e0 = c * ACCF_BLOCK;
        const AccfSpan s = accf_chunk_span(e0, R, cells);                                        // count <= ACCF_BLOCK + 2R
        for (int64_t t = threadIdx.x; t < s.count; t += ACCF_BLOCK) lds[t] = in[s.first + t];
        __syncthreads();
        const int64_t e = e0 + threadIdx.x;
        if (e < cells) {
            const int64_t i = e % len, base = e - i;                                             // the line's cells are [base, base + len)
            // the window [max(i - R, 0), min(i + R, len - 1)] of the line is cells [e - R, e + R] cut to the line: all of it is staged
            near += accf_store<LAST>(accf_line_min(lds, 1, s.first - base, s.count, len, i, R), e, R, out, last);
            all += 1;
        }
        __syncthreads();
    }
    if (LAST) {
        accum_wave_count(counters, ACCF_C_NEAR, near);
        accum_wave_count(counters, ACCF_C_FAR, all - near);
    }
}

static __global__ __launch_bounds__(ACCF_BLOCK) void accf_lookup_kernel(const float *__restrict__ points, const int32_t *__restrict__ coords, int64_t n,
                                                                         const double *__restrict__ pose, double voxel_size, AccfBox box, int64_t cells,
                                                                         const int32_t *__restrict__ dist2, const int32_t *__restrict__ nearest,
                                                                         uint8_t *__restrict__ out_status, int32_t *__restrict__ out_dist2,
                                                                         int32_t *__restrict__ out_row, u64 *__restrict__ counters)
{
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    long long c_rows = 0, c_valid = 0, c_inside = 0, c_near = 0;
    for (int64_t i = (int64_t)blockIdx.x * ACCF_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ACCF_BLOCK) {
        int32_t c[3] = {0, 0, 0};
        bool valid;
        if (points) {
            const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
            unsigned long long key = 0;
            int64_t q[3];
            valid = accum_point(T, p, voxel_size, &key, q);
            if (valid) accum_unkey(key, c);
        } else {
            c[0] = coords[3 * i]; c[1] = coords[3 * i + 1]; c[2] = coords[3 * i + 2];
            valid = accf_coord_valid(c);
        }
        int32_t d2, row;
        const int status = accf_lookup(valid, c, box, cells, dist2, nearest, &d2, &row);
        out_status[i] = (uint8_t)status; out_dist2[i] = d2; out_row[i] = row;
        c_rows += 1; c_valid += (status & ACCF_VALID) != 0; c_inside += (status & ACCF_INSIDE) != 0; c_near += (status & ACCF_NEAR) != 0;
    }
    accum_wave_count(counters, PCACC_FIELD_LOOKUP_ROWS, c_rows);
    accum_wave_count(counters, PCACC_FIELD_LOOKUP_N_VALID, c_valid);
    accum_wave_count(counters, PCACC_FIELD_LOOKUP_N_INSIDE, c_inside);
    accum_wave_count(counters, PCACC_FIELD_LOOKUP_N_NEAR, c_near);
}

struct AccfWs { AccnRowsWs rows; u64 *a, *b; };

// m = 0 carves as m = 1.  -> bytes taken: the row table of pass 1 and two grids of packed values.
static size_t accf_ws_carve(int64_t m, int64_t cells, AccfWs *w, char *base)
{
    size_t off = accn_rows_ws_carve(m, &w->rows, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->a = (u64 *)take((size_t)cells * 8);
    w->b = (u64 *)take((size_t)cells * 8);
    return off;
}

// One pass from `in` to `out` (or, the last one, to the two outputs).
template <bool LAST>
static void accf_pass(const u64 *in, int64_t cells, int64_t stride, int64_t len, int R, u64 *out, AccfOut last, u64 *counters, hipStream_t st)
{
    if (stride == 1) {
        const int grid = pcacc_grid(cells, ACCF_BLOCK, 1 << 20);
        hipLaunchKernelGGL(accf_line_kernel<LAST>, dim3(grid), dim3(ACCF_BLOCK), 0, st, in, cells, len, R, out, last, counters);
    } else {
        // a wave sums its counts over all its cells before its atomics: a grid that just fills the device (accum_columns.hip)
        hipLaunchKernelGGL(accf_direct_kernel<LAST>, dim3(pcacc_grid(cells, ACCF_BLOCK, LAST ? PCACC_CUS * 8 : 1 << 20)), dim3(ACCF_BLOCK), 0, st, in, cells,
                           stride, len, R, out, last, counters);
    }
}

extern "C" int pcacc_accum_field_workspace_bytes(int64_t m, int64_t cells, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY || cells < 1 || cells > ACCF_MAX_CELLS) return PCACC_E_ARG;
    AccfWs w;
    *bytes = accf_ws_carve(m, cells, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_field(const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                                 double max_moving_fraction, int64_t x0, int64_t y0, int64_t z0, int64_t nx, int64_t ny, int64_t nz, int32_t max_radius,
                                 int32_t planar, int32_t *out_dist2, int32_t *out_nearest, int64_t *counters, void *workspace, size_t workspace_bytes,
                                 void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || !counters || !workspace || !out_dist2 || !out_nearest) return PCACC_E_ARG;
    if (max_radius < 1 || max_radius > ACCF_MAX_RADIUS) return PCACC_E_ARG;
    const AccfBox box = {x0, y0, z0, nx, ny, nz, planar != 0 ? 1 : 0};
    const int64_t cells = accf_cells(box);
    if (cells < 1) return PCACC_E_ARG;
    if (m > 0 && (!keys || !acc)) return PCACC_E_ARG;
    AccfWs w;
    if (workspace_bytes < accf_ws_carve(m, cells, &w, (char *)workspace)) return PCACC_E_ARG;
    const void *outs[3] = {out_dist2, out_nearest, counters};
    const size_t bytes[3] = {4 * (size_t)cells, 4 * (size_t)cells, ACCF_COUNTERS * sizeof(int64_t)};
    const void *tab[2] = {keys, acc};
    const size_t tab_bytes[2] = {8 * (size_t)capacity, 8 * ACC_FIELDS * (size_t)capacity};
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 2; ++b)
            if (accum_bytes_overlap(outs[a], bytes[a], tab[b], tab_bytes[b])) return PCACC_E_ARG;
        for (int b = a + 1; b < 3; ++b)
            if (accum_bytes_overlap(outs[a], bytes[a], outs[b], bytes[b])) return PCACC_E_ARG;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCF_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) {                                                                                // all -1 and zero counters
        if (hipMemsetAsync(out_dist2, 0xff, 4 * (size_t)cells, st) != hipSuccess || hipMemsetAsync(out_nearest, 0xff, 4 * (size_t)cells, st) != hipSuccess)
            return PCACC_E_LAUNCH;
        return PCACC_OK;
    }
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows.rows, w.rows.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    if (hipMemsetAsync(w.a, 0xff, 8 * (size_t)cells, st) != hipSuccess) return PCACC_E_LAUNCH;   // every cell: none
    AcccMap M;
    M.keys = (const unsigned long long *)keys; M.acc = acc; M.stamps = nullptr; M.rows = w.rows.rows.rows;
    M.capacity = capacity; M.m = m; M.kept = 0;                                                // the kernel reads the kept count from the device
    u64 *cnt = (u64 *)counters;
    hipLaunchKernelGGL(accf_site_kernel, dim3(pcacc_grid(m, ACCF_BLOCK)), dim3(ACCF_BLOCK), 0, st, M, (const int64_t *)w.rows.kept, box, cells, w.a, cnt);
    PCACC_CHECK_LAUNCH();
    const int R = (int)max_radius;
    const int64_t nzo = accf_nz_out(box);
    const AccfOut last = {out_dist2, out_nearest}, none = {nullptr, nullptr};
    u64 *in = w.a, *out = w.b;
    if (!box.planar) {
        accf_pass<false>(in, cells, 1, nzo, R, out, none, cnt, st);               // z
        PCACC_CHECK_LAUNCH();
        u64 *t = in; in = out; out = t;
    }
    accf_pass<false>(in, cells, nzo, ny, R, out, none, cnt, st);                   // y
    PCACC_CHECK_LAUNCH();
    accf_pass<true>(out, cells, ny * nzo, nx, R, nullptr, last, cnt, st);          // x, the cut and the two outputs
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

extern "C" int pcacc_accum_field_lookup(const float *points, const int32_t *coords, int64_t n, const double *pose, double voxel_size, int64_t x0, int64_t y0,
                                        int64_t z0, int64_t nx, int64_t ny, int64_t nz, int32_t planar, const int32_t *dist2, const int32_t *nearest,
                                        uint8_t *out_status, int32_t *out_dist2, int32_t *out_row, int64_t *counters, void *stream)
{
    if (n < 0 || n > ACCF_MAX_POINTS || !counters || !dist2 || !nearest) return PCACC_E_ARG;
    if (!(voxel_size > 0.0) || !(voxel_size - voxel_size == 0.0)) return PCACC_E_ARG;
    const AccfBox box = {x0, y0, z0, nx, ny, nz, planar != 0 ? 1 : 0};
    const int64_t cells = accf_cells(box);
    if (cells < 1) return PCACC_E_ARG;
    if (n > 0 && ((points != nullptr) == (coords != nullptr))) return PCACC_E_ARG;               // exactly one of the two
    if (n > 0 && (!out_status || !out_dist2 || !out_row)) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCF_LOOKUP_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;   // written, not added to
    if (n == 0) return PCACC_OK;
    hipLaunchKernelGGL(accf_lookup_kernel, dim3(pcacc_grid(n, ACCF_BLOCK)), dim3(ACCF_BLOCK), 0, st, points, coords, n, pose, voxel_size, box, cells, dist2,
                       nearest, out_status, out_dist2, out_row, (u64 *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
