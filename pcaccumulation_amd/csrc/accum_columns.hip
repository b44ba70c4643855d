// C17. The (x, y) columns of the accumulated scene cloud: ground, height above ground and bird's-eye-view rasters (include/pcacc.h C17, DESIGN.md
// section 9q).
//
// The map of accum.hip is a sorted key list whose low 21 bits are z: the kept voxels of one (x, y) are consecutive rows of extract().  No sort, no hash.
//   rows     pass 1 of C5 (accn_rows_launch): dst[m], rows[kept] its inverse; the kept count stays on the device.
//   heads    head[j] = accc_is_head over the kept rows (0 behind them), then pcacc_scan_i32: cpos[j] = heads in front of j, cpos[m] = C, both on the
//            device.  The column of row j is cpos[j] + head[j] - 1 (accum_run_index).
//   columns  one lane per kept row; the lane of a head walks its run (accc_column): key, xy, first_row, voxels, sums, stamps, z_low / z_high.  Runs
//            are as long as the scene is tall in voxels; the other lanes of the wave wait for the longest of theirs.
//   ground   one lane per column: accc_ground -- per dx one accum_lower_bound in the compact column-key list and a walk over at most 2R + 1 columns.
//   rows     one lane per kept row: column, height, is_ground, height_m; the lane of a head also walks its run for the band (accc_band).
//   pixels   a separate entry: pass 1 of C5 again (a pixel reads the z centroid of two rows of extract()), then one lane per pixel: one binary
//            search of its column key (accc_pixel), then the gathers.  Every pixel is written once by its lane.
// The functions named are those of accum_columns.h -- the code the host build runs with every index assert-checked.  No floating-point atomics, no
// LDS beyond the scan's, no inline assembly; the five counts are summed per lane, reduced over the wave, one integer atomic per wave and non-zero
// counter (accum_wave_count).  Every result is an integer or one fixed sequence of IEEE operations: two runs give the same bits.
#include "scan.h"
#include "accum_columns.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACCC_BLOCK 256

static_assert(ACCC_MAX_RADIUS == PCACC_COLUMNS_MAX_RADIUS && ACCC_MAX_HEIGHT == PCACC_COLUMNS_MAX_HEIGHT && ACCC_MAX_PIXELS == PCACC_BEV_MAX_PIXELS &&
              ACCC_COUNTERS == PCACC_COLUMNS_COUNTERS && ACCC_C_ROWS == PCACC_COLUMNS_N_ROWS && ACCC_C_COLUMNS == PCACC_COLUMNS_N_COLUMNS &&
              ACCC_C_GROUND == PCACC_COLUMNS_N_GROUND && ACCC_C_BAND == PCACC_COLUMNS_N_BAND && ACCC_C_BORROWED == PCACC_COLUMNS_N_BORROWED,
              "accum_columns.h and include/pcacc.h name the same limits and counters");

struct AcccColumnOut {                                // [m] each, xy [m][2]; the first C rows are written
    int64_t *key;
    int32_t *xy, *first_row, *voxels;
    int64_t *points, *moving;
    int32_t *z_low, *z_high, *t_first, *t_last, *ground_z, *ground_row, *ground_column, *band_voxels, *band_top;
};

struct AcccRowOut {                                   // [m] each; the first kept rows are written
    int32_t *column, *height;
    uint8_t *is_ground;
    double *height_m;
};

// The kept count and the number of columns as the device holds them, cut to what the tables have room for.
static __device__ __forceinline__ int64_t accc_kept(const int64_t *kept_ptr, int64_t m)
{
    const int64_t kept = *kept_ptr;
    return kept < 0 ? 0 : (kept > m ? m : kept);
}

static __device__ __forceinline__ int64_t accc_columns(const int *cpos, int64_t m, int64_t kept)
{
    const int64_t C = cpos[m];
    return C < 0 ? 0 : (C > kept ? kept : C);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_head_kernel(AcccMap M, const int64_t *__restrict__ kept_ptr, int *__restrict__ head)
{
    M.kept = accc_kept(kept_ptr, M.m);
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < M.m; j += (int64_t)gridDim.x * ACCC_BLOCK)
        head[j] = (j < M.kept && accc_is_head(M, j)) ? 1 : 0;                                   // 0 behind the kept rows: the scan runs over m entries
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_column_kernel(AcccMap M, const int64_t *__restrict__ kept_ptr, const int *__restrict__ head,
                                                                         const int *__restrict__ cpos, AcccColumnOut out, int64_t *__restrict__ out_n)
{
    M.kept = accc_kept(kept_ptr, M.m);
    const int64_t C = accc_columns(cpos, M.m, M.kept);
    if (blockIdx.x == 0 && threadIdx.x == 0) { out_n[0] = M.kept; out_n[1] = C; }
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < M.kept; j += (int64_t)gridDim.x * ACCC_BLOCK) {
        if (!head[j]) continue;
        const int64_t c = accum_run_index(cpos[j], 1, C);
        AcccColumn col;
        if (c < 0 || !accc_column(M, j, &col)) continue;
        out.key[c] = (int64_t)col.key;
        out.xy[2 * c] = col.xy[0]; out.xy[2 * c + 1] = col.xy[1];
        out.first_row[c] = col.first_row; out.voxels[c] = col.voxels;
        out.points[c] = col.points; out.moving[c] = col.moving;
        out.z_low[c] = col.z_low; out.z_high[c] = col.z_high;
        out.t_first[c] = col.t_first; out.t_last[c] = col.t_last;
    }
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_ground_kernel(const int64_t *__restrict__ kept_ptr, const int *__restrict__ cpos, int64_t m, int radius,
                                                                         AcccColumnOut out, unsigned long long *__restrict__ counters)
{
    const int64_t C = accc_columns(cpos, m, accc_kept(kept_ptr, m));
    long long columns = 0, borrowed = 0;
    for (int64_t c = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; c < C; c += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int64_t g = accc_ground((const unsigned long long *)out.key, out.z_low, C, c, radius);
        if (g < 0) continue;
        out.ground_z[c] = out.z_low[g];
        out.ground_row[c] = out.first_row[g];
        out.ground_column[c] = (int32_t)g;
        columns += 1;
        borrowed += g != c;
    }
    accum_wave_count(counters, ACCC_C_COLUMNS, columns);                                        // every lane of the wave arrives here
    accum_wave_count(counters, ACCC_C_BORROWED, borrowed);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_row_kernel(AcccMap M, const int64_t *__restrict__ kept_ptr, const int *__restrict__ head,
                                                                      const int *__restrict__ cpos, int thickness, int band_lo, int band_hi,
                                                                      AcccColumnOut col, AcccRowOut out, unsigned long long *__restrict__ counters)
{
#pragma clang fp contract(off)
    M.kept = accc_kept(kept_ptr, M.m);
    const int64_t C = accc_columns(cpos, M.m, M.kept);
    long long rows = 0, ground = 0, band = 0;
    for (int64_t j = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; j < M.kept; j += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int h = head[j];
        const int64_t c = accum_run_index(cpos[j], h, C);
        int32_t z;
        if (c < 0 || !accc_row_z(M, j, &z)) continue;
        const int32_t gz = col.ground_z[c], height = z - gz;
        out.column[j] = (int32_t)c;
        out.height[j] = height;
        out.is_ground[j] = height <= thickness ? 1 : 0;
        out.height_m[j] = accc_height_m(M, j, col.ground_row[c]);
        rows += 1;
        ground += height <= thickness;
        if (h) {                                                                                 // the head's lane owns the column's band
            int32_t top;
            const int32_t n = accc_band(M, j, col.voxels[c], gz, band_lo, band_hi, &top);
            col.band_voxels[c] = n;
            col.band_top[c] = top;
            band += n;
        }
    }
    accum_wave_count(counters, ACCC_C_ROWS, rows);
    accum_wave_count(counters, ACCC_C_GROUND, ground);
    accum_wave_count(counters, ACCC_C_BAND, band);
}

static __global__ __launch_bounds__(ACCC_BLOCK) void accc_pixel_kernel(AcccMap M, const int64_t *__restrict__ kept_ptr, AcccColumns T, int64_t x0, int64_t y0,
                                                                        int64_t W, int64_t H, int32_t *__restrict__ out_column, float *__restrict__ out_elevation,
                                                                        float *__restrict__ out_ground, int32_t *__restrict__ out_band_top,
                                                                        int32_t *__restrict__ out_voxels)
{
    M.kept = kept_ptr ? accc_kept(kept_ptr, M.m) : 0;
    const int64_t n = W * H;
    for (int64_t p = (int64_t)blockIdx.x * ACCC_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * ACCC_BLOCK) {
        const int64_t r = p / W, c = p - r * W;
        AcccPixel px;
        accc_pixel(M, T, x0 + c, y0 + r, &px);
        out_column[p] = px.column;
        out_elevation[p] = px.elevation;
        out_ground[p] = px.ground;
        out_band_top[p] = px.band_top;
        out_voxels[p] = px.voxels;
    }
}

struct AcccWs { AccnRowsWs rows; int *head, *cpos, *chunk; };

// m = 0 carves as m = 1.  -> bytes taken.
static size_t accc_ws_carve(int64_t m, AcccWs *w, char *base)
{
    const int64_t n = m > 0 ? m : 1;
    size_t off = accn_rows_ws_carve(m, &w->rows, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->head = (int *)take((size_t)n * 4);
    w->cpos = (int *)take((size_t)(n + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(n) * 4);
    return off;
}

// Some output table shares a byte with a table of the map.
static bool accc_overlaps_map(const void *const *outs, const size_t *bytes, int n_outs, const void *keys, const void *acc, const void *stamps, int64_t capacity)
{
    const void *tab[3] = {keys, acc, stamps};
    const size_t row_bytes[3] = {8, 8 * ACC_FIELDS, 4 * 2};
    for (int a = 0; a < n_outs; ++a)
        for (int b = 0; b < 3; ++b)
            if (accum_bytes_overlap(outs[a], bytes[a], tab[b], row_bytes[b] * (size_t)capacity)) return true;
    return false;
}

extern "C" int pcacc_accum_columns_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AcccWs w;
    *bytes = accc_ws_carve(m, &w, nullptr);
    return PCACC_OK;
}

extern "C" int pcacc_accum_columns(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                                   int32_t use_fraction, double max_moving_fraction, int32_t ground_radius, int32_t thickness, int32_t band_lo,
                                   int32_t band_hi, int64_t *col_key, int32_t *col_xy, int32_t *col_first_row, int32_t *col_voxels, int64_t *col_points,
                                   int64_t *col_moving, int32_t *col_z_low, int32_t *col_z_high, int32_t *col_t_first, int32_t *col_t_last,
                                   int32_t *col_ground_z, int32_t *col_ground_row, int32_t *col_ground_column, int32_t *col_band_voxels,
                                   int32_t *col_band_top, int32_t *row_column, int32_t *row_height, uint8_t *row_is_ground, double *row_height_m,
                                   int64_t *out_n, int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || !out_n || !counters || !workspace) return PCACC_E_ARG;
    if (ground_radius < 0 || ground_radius > ACCC_MAX_RADIUS || thickness < 0 || thickness > ACCC_MAX_HEIGHT) return PCACC_E_ARG;
    if (band_lo < 0 || band_lo > band_hi || band_hi > ACCC_MAX_HEIGHT) return PCACC_E_ARG;
    const void *outs[19] = {col_key, col_xy, col_first_row, col_voxels, col_points, col_moving, col_z_low, col_z_high, col_t_first, col_t_last,
                            col_ground_z, col_ground_row, col_ground_column, col_band_voxels, col_band_top, row_column, row_height, row_is_ground,
                            row_height_m};
    const size_t width[19] = {8, 8, 4, 4, 8, 8, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 8};
    size_t bytes[19];
    for (int a = 0; a < 19; ++a) {
        if (m > 0 && !outs[a]) return PCACC_E_ARG;
        bytes[a] = width[a] * (size_t)m;
    }
    if (m > 0 && (!keys || !acc || !stamps)) return PCACC_E_ARG;
    AcccWs w;
    if (workspace_bytes < accc_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    const void *words[2] = {out_n, counters};
    const size_t word_bytes[2] = {2 * sizeof(int64_t), ACCC_COUNTERS * sizeof(int64_t)};
    if (accc_overlaps_map(outs, bytes, 19, keys, acc, stamps, capacity) || accc_overlaps_map(words, word_bytes, 2, keys, acc, stamps, capacity))
        return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACCC_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return hipMemsetAsync(out_n, 0, 2 * sizeof(int64_t), st) == hipSuccess ? PCACC_OK : PCACC_E_LAUNCH;
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows.rows, w.rows.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    AcccMap M;
    M.keys = (const unsigned long long *)keys; M.acc = acc; M.stamps = stamps; M.rows = w.rows.rows.rows;
    M.capacity = capacity; M.m = m; M.kept = 0;                                                // the kernels read the kept count from the device
    const AcccColumnOut col = {col_key, col_xy, col_first_row, col_voxels, col_points, col_moving, col_z_low, col_z_high, col_t_first, col_t_last,
                               col_ground_z, col_ground_row, col_ground_column, col_band_voxels, col_band_top};
    const AcccRowOut row = {row_column, row_height, row_is_ground, row_height_m};
    const int64_t *kept = w.rows.kept;
    const int *head = w.head, *cpos = w.cpos;
    const int grid = pcacc_grid(m, ACCC_BLOCK), wide = pcacc_grid(m, ACCC_BLOCK, 1 << 22);
    hipLaunchKernelGGL(accc_head_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, kept, w.head);
    pcacc_scan_i32(w.head, m, w.chunk, w.cpos, st);                                             // cpos[m] = C
    PCACC_CHECK_LAUNCH();
    // a head's lane walks its run while its wave waits: many small workgroups spread over the CUs, as accum_normals.hip
    hipLaunchKernelGGL(accc_column_kernel, dim3(wide), dim3(ACCC_BLOCK), 0, st, M, kept, head, cpos, col, out_n);
    PCACC_CHECK_LAUNCH();
    // the kernels that count run a grid-stride loop on a grid that just fills the device: a wave sums its counts over all its rows before its atomics.
    // On the wide grid 125 000 waves ended in three atomics on the same three words: the row kernel took 4.54 ms at 8 M rows instead of 0.65 ms
    // (profiles/accum_columns_bench.txt, the interleaved A/B)
    hipLaunchKernelGGL(accc_ground_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, kept, cpos, m, (int)ground_radius, col, (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    hipLaunchKernelGGL(accc_row_kernel, dim3(grid), dim3(ACCC_BLOCK), 0, st, M, kept, head, cpos, (int)thickness, (int)band_lo, (int)band_hi, col, row,
                       (unsigned long long *)counters);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}

extern "C" int pcacc_accum_bev(const int64_t *keys, const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int32_t use_fraction,
                               double max_moving_fraction, const int64_t *col_key, const int32_t *col_first_row, const int32_t *col_voxels,
                               const int32_t *col_ground_row, const int32_t *col_band_top, int64_t n_columns, int64_t x0, int64_t y0, int64_t width,
                               int64_t height, int32_t *out_column, float *out_elevation, float *out_ground, int32_t *out_band_top, int32_t *out_voxels,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || n_columns < 0 || n_columns > m || !workspace) return PCACC_E_ARG;
    if (width < 1 || height < 1 || width > ACCC_MAX_PIXELS || height > ACCC_MAX_PIXELS || width * height > ACCC_MAX_PIXELS) return PCACC_E_ARG;
    if (x0 < -ACCC_MAX_ORIGIN || x0 > ACCC_MAX_ORIGIN || y0 < -ACCC_MAX_ORIGIN || y0 > ACCC_MAX_ORIGIN) return PCACC_E_ARG;
    if (!out_column || !out_elevation || !out_ground || !out_band_top || !out_voxels) return PCACC_E_ARG;
    if (n_columns > 0 && (!keys || !acc || !col_key || !col_first_row || !col_voxels || !col_ground_row || !col_band_top)) return PCACC_E_ARG;
    AcccWs w;
    if (workspace_bytes < accc_ws_carve(m, &w, (char *)workspace)) return PCACC_E_ARG;
    const size_t n = (size_t)(width * height);
    const void *outs[5] = {out_column, out_elevation, out_ground, out_band_top, out_voxels};
    const size_t bytes[5] = {4 * n, 4 * n, 4 * n, 4 * n, 4 * n};
    if (accc_overlaps_map(outs, bytes, 5, keys, acc, nullptr, capacity)) return PCACC_E_ARG;
    const void *cols[5] = {col_key, col_first_row, col_voxels, col_ground_row, col_band_top};
    const size_t col_bytes[5] = {8 * (size_t)n_columns, 4 * (size_t)n_columns, 4 * (size_t)n_columns, 4 * (size_t)n_columns, 4 * (size_t)n_columns};
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            if (accum_bytes_overlap(outs[a], bytes[a], cols[b], col_bytes[b])) return PCACC_E_ARG;
    hipStream_t st = pcacc_stream(stream);
    const bool any = n_columns > 0;                                                             // no column: an all-empty image, no row is read
    if (any && accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows.rows, w.rows.kept, st) != PCACC_OK)
        return PCACC_E_LAUNCH;
    AcccMap M;
    M.keys = (const unsigned long long *)keys; M.acc = acc; M.stamps = nullptr; M.rows = w.rows.rows.rows;
    M.capacity = capacity; M.m = m; M.kept = 0;
    const AcccColumns T = {(const unsigned long long *)col_key, col_first_row, col_voxels, col_ground_row, col_band_top, n_columns};
    hipLaunchKernelGGL(accc_pixel_kernel, dim3(pcacc_grid((int64_t)n, ACCC_BLOCK, 1 << 20)), dim3(ACCC_BLOCK), 0, st, M,
                       any ? (const int64_t *)w.rows.kept : (const int64_t *)nullptr, T, x0, y0, width, height, out_column, out_elevation, out_ground,
                       out_band_top, out_voxels);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
