// C18. Planar segments of the accumulated scene cloud by normal-gated region growing, on the device (include/pcacc.h C18).
//
//   rows      pass 1 of C5 (accn_rows_launch): dst[m], extract's row of every map row, -1 = filtered out; rows[kept] its inverse; kept stays on the device.
//   class     parent[j] = j, and part[j] = extract row j takes part (acpl_class of accum_planes.h: filter, mask, valid normal, flat neighbourhood); the
//             five row counts, one integer atomic per wave and non-zero counter.  Tables that do not fit the kept count: BAD_ROWS, part = 0 everywhere,
//             and no later kernel reads a normal or the mask.
//   link      one lane per extract row in a grid-stride loop: accc_edges of C11 with `part` as its mask names every pair once from its larger end,
//             acpl_joined decides it, uf_union_bounded joins (GAVE_UP after ACCC_UNION_TRIES lost attempts).
//   flatten   parent[j] = root of j; a slot is written by its own lane only (uf_root stores nothing on its way).
//   number    root flags -> scan.h -> segment number in ascending order of the smallest row.  The lane of row j writes label[j]; the lane of a root
//             also writes first_row, the anchor A and the neutral elements of its segment's record.
//   pass 1    accc_stat_row and |u - A| of each row, an inclusive segmented scan over runs of equal label among consecutive lanes
//             (accc_stat_merge), one integer atomic per (wave, run) and field; D by a 64-bit unsigned atomicMax.
//   shift     one lane per segment: voxels, s = acpl_shift(D, voxels), the largest segment by a wave maximum.
//   pass 2    acpl_moments_row of each row, the same run reduction, nine 64-bit integer atomicAdd per (wave, run).
//   fit       one lane per segment: acpl_fit.
//   distance  one lane per extract row: acpl_distance to the plane of its own segment.
// Nothing is read back.  No floating-point atomics, no LDS beyond the scan's, no inline assembly; the map is read only.
#include "scan.h"
#include "accum_planes.h"
#include "accum_launch.h"
#include "accum_rows.h"

#define ACPL_BLOCK 256

static_assert(ACPL_COUNTERS == PCACC_PLANES_COUNTERS && ACPL_C_ROWS == PCACC_PLANES_ROWS && ACPL_C_PARTICIPATING == PCACC_PLANES_PARTICIPATING &&
              ACPL_C_OUTSIDE == PCACC_PLANES_OUTSIDE && ACPL_C_MASKED == PCACC_PLANES_MASKED && ACPL_C_INVALID == PCACC_PLANES_INVALID &&
              ACPL_C_NOT_FLAT == PCACC_PLANES_NOT_FLAT && ACPL_C_SEGMENTS == PCACC_PLANES_K && ACPL_C_LARGEST == PCACC_PLANES_LARGEST &&
              ACPL_C_STATUS == PCACC_PLANES_STATUS && ACPL_OK == PCACC_PLANES_OK && ACPL_BAD_ROWS == PCACC_PLANES_BAD_ROWS &&
              ACPL_GAVE_UP == PCACC_PLANES_GAVE_UP && ACPL_PLANE_DEGENERATE == PCACC_PLANE_DEGENERATE,
              "accum_planes.h and include/pcacc.h name the same counters and codes");

struct AcplMap {                         // named scalars: nothing here is indexed at run time
    const unsigned long long *keys;
    const int64_t *acc;
    const int32_t *stamps;
    const float *normals, *eigenvalues;
    const uint8_t *flags, *mask;
    const int *dst, *rows;
    const int64_t *kept;
    int64_t capacity, m, mask_rows, n_rows;
    double cos_angle, max_offset, max_variation;
    int radius;
};

struct AcplOut {
    int32_t *label;
    double *distance;
    int32_t *voxels;
    int64_t *points;
    int32_t *lo, *hi, *first_row, *t_first, *t_last, *anchor;
    int64_t *spread;
    int32_t *shift;
    int64_t *s1, *s2;
    double *normal, *eigenvalues, *centroid, *offset, *mse;
    uint8_t *flags;
    unsigned long long *counters;
};

static __device__ __forceinline__ int64_t acpl_kept(const AcplMap &M)
{
    const int64_t kept = *M.kept;
    return kept > M.m ? M.m : (kept < 0 ? 0 : kept);
}

// The number of segments as the label kernel left it, never above the rows a table has.
static __device__ __forceinline__ int64_t acpl_segments(const AcplOut &out, int64_t rows)
{
    const int64_t k = (int64_t)out.counters[ACPL_C_SEGMENTS];
    return k > rows ? rows : (k < 0 ? 0 : k);
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_class_kernel(AcplMap M, int *__restrict__ parent, uint8_t *__restrict__ part,
                                                                        unsigned long long *__restrict__ counters)
{
    const int64_t kept = acpl_kept(M);
    const bool fits = acpl_rows_fit(M.mask, M.mask_rows, M.n_rows, kept);                     // uniform over the grid
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                               // the memset left 0; no lane adds to these
        counters[ACPL_C_ROWS] = (unsigned long long)M.m;
        counters[ACPL_C_OUTSIDE] = (unsigned long long)(M.m - kept);
        if (!fits) {
            counters[ACPL_C_MASKED] = (unsigned long long)kept;
            counters[ACPL_C_STATUS] = ACPL_BAD_ROWS;
        }
    }
    long long c_part = 0, c_masked = 0, c_invalid = 0, c_rough = 0;
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < M.m; j += (int64_t)gridDim.x * ACPL_BLOCK) {
        parent[j] = (int)j;
        int cls = ACPL_OUTSIDE;
        if (fits && j < kept) cls = acpl_class(M.mask, M.flags, M.eigenvalues, kept, j, M.max_variation);
        part[j] = cls == ACPL_TAKES_PART ? 1 : 0;
        c_part += cls == ACPL_TAKES_PART; c_masked += cls == ACPL_MASKED; c_invalid += cls == ACPL_INVALID; c_rough += cls == ACPL_NOT_FLAT;
    }
    // every lane of the wave arrives here: one atomic per wave and non-zero counter
    accum_wave_count(counters, ACPL_C_PARTICIPATING, c_part);
    accum_wave_count(counters, ACPL_C_MASKED, c_masked);
    accum_wave_count(counters, ACPL_C_INVALID, c_invalid);
    accum_wave_count(counters, ACPL_C_NOT_FLAT, c_rough);
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_link_kernel(AcplMap M, const uint8_t *__restrict__ part, int *__restrict__ parent,
                                                                       unsigned long long *__restrict__ counters)
{
    const int64_t kept = acpl_kept(M);
    if (!acpl_rows_fit(M.mask, M.mask_rows, M.n_rows, kept)) return;
    bool gave_up = false;
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACPL_BLOCK) {
        const int64_t i = M.rows[j];
        if (i < 0 || i >= M.m || M.dst[i] != j) continue;                                    // a table that does not fit addresses nothing
        AcplRow mine;
        if (!accc_takes_part(part, kept, j) || !acpl_row(M.acc, M.capacity, M.m, i, M.normals, kept, j, &mine)) continue;
        accc_edges(M.keys, M.m, M.dst, part, kept, i, j, M.radius, [&](int64_t a, int64_t b) {
            const int64_t q = accn_index(b, kept);
            const int64_t p = q < 0 ? -1 : accn_index(M.rows[q], M.m);
            AcplRow other;
            if (p < 0 || !acpl_row(M.acc, M.capacity, M.m, p, M.normals, kept, q, &other)) return;
            if (!acpl_joined(mine, other, M.cos_angle, M.max_offset)) return;
            if (uf_union_bounded(parent, (int)a, (int)q, ACCC_UNION_TRIES) < 0) gave_up = true;
        });
    }
    if (gave_up) atomicMax(&counters[ACPL_C_STATUS], (unsigned long long)ACPL_GAVE_UP);
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_flatten_kernel(AcplMap M, int *__restrict__ parent)
{
    const int64_t kept = acpl_kept(M);
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACPL_BLOCK) {
        const int r = uf_root(parent, (int)j);
        if (r != (int)j) uf_store(&parent[j], r);
    }
}

// flag[j] = extract row j is the root of a segment; 0 for every slot behind kept (the scan runs over m slots).
static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_root_kernel(AcplMap M, const uint8_t *__restrict__ part, const int *__restrict__ parent,
                                                                       int *__restrict__ flag)
{
    const int64_t kept = acpl_kept(M);
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < M.m; j += (int64_t)gridDim.x * ACPL_BLOCK)
        flag[j] = (j < kept && accc_takes_part(part, kept, j) && parent[j] == (int)j) ? 1 : 0;
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_label_kernel(AcplMap M, const uint8_t *__restrict__ part, const int *__restrict__ parent,
                                                                        const int *__restrict__ cid, AcplOut out, unsigned long long *__restrict__ vox64)
{
    const int64_t kept = acpl_kept(M);
    int64_t n_seg = cid[M.m];
    n_seg = n_seg > kept ? kept : (n_seg < 0 ? 0 : n_seg);                                   // K against kept before a table is addressed
    if (blockIdx.x == 0 && threadIdx.x == 0) out.counters[ACPL_C_SEGMENTS] = (unsigned long long)n_seg;
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACPL_BLOCK) {
        int32_t lab = -1;
        if (accc_takes_part(part, kept, j)) {
            const int64_t root = accn_index(parent[j], kept);
            const int64_t c = root < 0 ? -1 : accn_index(cid[root], n_seg);
            lab = (int32_t)c;
            if (c >= 0 && root == j) {                                                       // the root's lane: the neutral record of segment c
                int64_t ux = 0, uy = 0, uz = 0;
                const int64_t i = M.rows[j];
                if (i >= 0 && i < M.m && M.dst[i] == j) acpl_int_centroid(M.acc, M.capacity, M.m, i, &ux, &uy, &uz);
                out.first_row[c] = (int32_t)j;
                out.anchor[3 * c] = (int32_t)ux; out.anchor[3 * c + 1] = (int32_t)uy; out.anchor[3 * c + 2] = (int32_t)uz;
                vox64[c] = 0; out.points[c] = 0; out.spread[c] = 0;
                out.lo[3 * c] = ACCC_I32_MAX; out.lo[3 * c + 1] = ACCC_I32_MAX; out.lo[3 * c + 2] = ACCC_I32_MAX;
                out.hi[3 * c] = ACCC_I32_MIN; out.hi[3 * c + 1] = ACCC_I32_MIN; out.hi[3 * c + 2] = ACCC_I32_MIN;
                out.t_first[c] = ACCC_I32_MAX; out.t_last[c] = ACCC_I32_MIN;
                for (int k = 0; k < 3; ++k) out.s1[3 * c + k] = 0;
                for (int k = 0; k < 6; ++k) out.s2[6 * c + k] = 0;
            }
        }
        out.label[j] = lab;
    }
}

// Runs of equal label among the 64 consecutive lanes of a wave: *start = the first lane of this lane's run, *tail = this lane ends its run.
static __device__ __forceinline__ void acpl_runs(int lab, int lane, int *start, bool *tail)
{
    const int before = __shfl_up(lab, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != lab);
    *start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    *tail = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0;
}

static __device__ __forceinline__ void acpl_stat_from_lane(AcccStat *o, const AcccStat &s, int d)
{
    o->voxels = __shfl_up((long long)s.voxels, d, 64); o->points = __shfl_up((long long)s.points, d, 64);
    o->moving = 0; o->sq_x = 0; o->sq_y = 0; o->sq_z = 0;                                     // not part of a segment's record
    o->lo_x = __shfl_up(s.lo_x, d, 64); o->lo_y = __shfl_up(s.lo_y, d, 64); o->lo_z = __shfl_up(s.lo_z, d, 64);
    o->hi_x = __shfl_up(s.hi_x, d, 64); o->hi_y = __shfl_up(s.hi_y, d, 64); o->hi_z = __shfl_up(s.hi_z, d, 64);
    o->t_first = __shfl_up(s.t_first, d, 64); o->t_last = __shfl_up(s.t_last, d, 64);
}

// The map row and the label of extract row j, or -1 when either names nothing.
static __device__ __forceinline__ int acpl_member(const AcplMap &M, const AcplOut &out, int64_t kept, int64_t n_seg, int64_t j, int64_t *row)
{
    *row = -1;
    if (j >= kept) return -1;
    const int64_t i = M.rows[j];
    const int l = out.label[j];
    if (l < 0 || l >= n_seg || i < 0 || i >= M.m || M.dst[i] != j) return -1;
    *row = i;
    return l;
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_stats_kernel(AcplMap M, AcplOut out, unsigned long long *__restrict__ vox64)
{
    const int64_t kept = acpl_kept(M);
    const int64_t n_seg = acpl_segments(out, kept);                                          // written by the launch before this one
    const int lane = lane_id();
    for (int64_t base = (int64_t)blockIdx.x * ACPL_BLOCK; base < kept; base += (int64_t)gridDim.x * ACPL_BLOCK) {      // uniform: all 64 lanes shuffle
        int64_t i;
        int lab = acpl_member(M, out, kept, n_seg, base + threadIdx.x, &i);
        AcccStat s;
        accc_stat_none(&s);
        unsigned long long spread = 0;
        if (lab >= 0) {
            int64_t ux, uy, uz;
            if (accc_stat_row(M.keys, M.acc, M.stamps, M.capacity, M.m, i, &s) && acpl_int_centroid(M.acc, M.capacity, M.m, i, &ux, &uy, &uz))
                spread = acpl_spread(ux, uy, uz, out.anchor[3 * lab], out.anchor[3 * lab + 1], out.anchor[3 * lab + 2]);
            else
                lab = -1;
        }
        int start;
        bool tail;
        acpl_runs(lab, lane, &start, &tail);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            AcccStat o;
            acpl_stat_from_lane(&o, s, d);
            const unsigned long long od = __shfl_up(spread, d, 64);
            if (lane - d >= start) {
                accc_stat_merge(&s, o);
                spread = od > spread ? od : spread;
            }
        }
        if (tail && lab >= 0) {
            const int64_t c = lab;
            atomicAdd(&vox64[c], (unsigned long long)s.voxels);
            atomicAdd((unsigned long long *)&out.points[c], (unsigned long long)s.points);
            atomicMin(&out.lo[3 * c], s.lo_x); atomicMin(&out.lo[3 * c + 1], s.lo_y); atomicMin(&out.lo[3 * c + 2], s.lo_z);
            atomicMax(&out.hi[3 * c], s.hi_x); atomicMax(&out.hi[3 * c + 1], s.hi_y); atomicMax(&out.hi[3 * c + 2], s.hi_z);
            atomicMin(&out.t_first[c], s.t_first);
            atomicMax(&out.t_last[c], s.t_last);
            atomicMax((unsigned long long *)&out.spread[c], spread);
        }
    }
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_shift_kernel(int64_t m, AcplOut out, const unsigned long long *__restrict__ vox64)
{
    const int64_t n_seg = acpl_segments(out, m);
    long long largest = 0;
    for (int64_t c = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; c < n_seg; c += (int64_t)gridDim.x * ACPL_BLOCK) {
        const long long v = (long long)vox64[c];
        out.voxels[c] = (int32_t)v;
        out.shift[c] = acpl_shift((uint64_t)out.spread[c], v);
        largest = v > largest ? v : largest;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(largest, d, 64);
        largest = o > largest ? o : largest;
    }
    if (lane_id() == 0 && largest > 0) atomicMax(&out.counters[ACPL_C_LARGEST], (unsigned long long)largest);
}

static __device__ __forceinline__ void acpl_moments_from_lane(AcplMoments *o, const AcplMoments &q, int d)
{
    o->x = __shfl_up((long long)q.x, d, 64); o->y = __shfl_up((long long)q.y, d, 64); o->z = __shfl_up((long long)q.z, d, 64);
    o->xx = __shfl_up((long long)q.xx, d, 64); o->xy = __shfl_up((long long)q.xy, d, 64); o->xz = __shfl_up((long long)q.xz, d, 64);
    o->yy = __shfl_up((long long)q.yy, d, 64); o->yz = __shfl_up((long long)q.yz, d, 64); o->zz = __shfl_up((long long)q.zz, d, 64);
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_moments_kernel(AcplMap M, AcplOut out)
{
    const int64_t kept = acpl_kept(M);
    const int64_t n_seg = acpl_segments(out, kept);
    const int lane = lane_id();
    for (int64_t base = (int64_t)blockIdx.x * ACPL_BLOCK; base < kept; base += (int64_t)gridDim.x * ACPL_BLOCK) {      // uniform: all 64 lanes shuffle
        int64_t i;
        int lab = acpl_member(M, out, kept, n_seg, base + threadIdx.x, &i);
        AcplMoments q;
        acpl_moments_none(&q);
        if (lab >= 0) {
            int64_t ux, uy, uz;
            if (acpl_int_centroid(M.acc, M.capacity, M.m, i, &ux, &uy, &uz))
                acpl_moments_row(ux, uy, uz, out.anchor[3 * lab], out.anchor[3 * lab + 1], out.anchor[3 * lab + 2], out.shift[lab], &q);
            else
                lab = -1;
        }
        int start;
        bool tail;
        acpl_runs(lab, lane, &start, &tail);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            AcplMoments o;
            acpl_moments_from_lane(&o, q, d);
            if (lane - d >= start) acpl_moments_merge(&q, o);
        }
        if (tail && lab >= 0) {
            unsigned long long *s1 = (unsigned long long *)&out.s1[3 * (int64_t)lab], *s2 = (unsigned long long *)&out.s2[6 * (int64_t)lab];
            atomicAdd(&s1[0], (unsigned long long)q.x); atomicAdd(&s1[1], (unsigned long long)q.y); atomicAdd(&s1[2], (unsigned long long)q.z);
            atomicAdd(&s2[0], (unsigned long long)q.xx); atomicAdd(&s2[1], (unsigned long long)q.xy); atomicAdd(&s2[2], (unsigned long long)q.xz);
            atomicAdd(&s2[3], (unsigned long long)q.yy); atomicAdd(&s2[4], (unsigned long long)q.yz); atomicAdd(&s2[5], (unsigned long long)q.zz);
        }
    }
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_fit_kernel(int64_t m, AcplOut out)
{
    const int64_t n_seg = acpl_segments(out, m);
    for (int64_t c = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; c < n_seg; c += (int64_t)gridDim.x * ACPL_BLOCK) {
        AcplFit f;
        acpl_fit(&out.anchor[3 * c], out.shift[c], out.voxels[c], &out.s1[3 * c], &out.s2[6 * c], &f);
        for (int k = 0; k < 3; ++k) {
            out.normal[3 * c + k] = f.normal[k];
            out.eigenvalues[3 * c + k] = f.eigenvalues[k];
            out.centroid[3 * c + k] = f.centroid[k];
        }
        out.offset[c] = f.offset;
        out.mse[c] = f.mse;
        out.flags[c] = (uint8_t)f.flags;
    }
}

static __global__ __launch_bounds__(ACPL_BLOCK) void acpl_distance_kernel(AcplMap M, AcplOut out)
{
    const int64_t kept = acpl_kept(M);
    const int64_t n_seg = acpl_segments(out, kept);
    for (int64_t j = (int64_t)blockIdx.x * ACPL_BLOCK + threadIdx.x; j < kept; j += (int64_t)gridDim.x * ACPL_BLOCK) {
        int64_t i;
        const int lab = acpl_member(M, out, kept, n_seg, j, &i);
        double d = 0.0;
        if (lab >= 0 && (out.flags[lab] & ACPL_PLANE_DEGENERATE) == 0)
            d = acpl_distance(M.acc, M.capacity, M.m, i, out.normal[3 * lab], out.normal[3 * lab + 1], out.normal[3 * lab + 2], out.offset[lab]);
        out.distance[j] = d;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------
struct AcplWs : AccnRowsWs { int *parent, *flag, *cid, *chunk; unsigned long long *vox64; uint8_t *part; };

static size_t acpl_carve(AcplWs *w, char *base, int64_t m)                                   // m >= 1
{
    size_t off = accn_rows_ws_carve(m, w, base);
    auto take = [&](size_t bytes) { char *p = base + off; off += pcacc_align(bytes); return p; };
    w->parent = (int *)take((size_t)m * 4);
    w->flag = (int *)take((size_t)m * 4);
    w->cid = (int *)take((size_t)(m + 1) * 4);
    w->chunk = (int *)take((size_t)pcacc_chunks(m) * 4);
    w->vox64 = (unsigned long long *)take((size_t)m * 8);
    w->part = (uint8_t *)take((size_t)m);
    return off;
}

extern "C" int pcacc_accum_planes_workspace_bytes(int64_t m, size_t *bytes)
{
    if (!bytes || m < 0 || m > ACCUM_MAX_CAPACITY) return PCACC_E_ARG;
    AcplWs w;
    *bytes = acpl_carve(&w, nullptr, m > 0 ? m : 1);
    return PCACC_OK;
}

extern "C" int pcacc_accum_planes(const int64_t *keys, const int64_t *acc, const int32_t *stamps, int64_t capacity, int64_t m, int64_t min_count,
                                  int32_t use_fraction, double max_moving_fraction, const float *normals, const float *eigenvalues, const uint8_t *flags,
                                  int64_t n_rows, const uint8_t *mask, int64_t mask_rows, int32_t radius, double cos_angle, double max_offset,
                                  double max_variation, int32_t *out_label, double *out_distance, int32_t *out_voxels, int64_t *out_points,
                                  int32_t *out_lo, int32_t *out_hi, int32_t *out_first_row, int32_t *out_t_first, int32_t *out_t_last,
                                  int32_t *out_anchor, int64_t *out_spread, int32_t *out_shift, int64_t *out_s1, int64_t *out_s2, double *out_normal,
                                  double *out_eigenvalues, double *out_centroid, double *out_offset, double *out_mse, uint8_t *out_flags,
                                  int64_t *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 0 || capacity < m || capacity > ACCUM_MAX_CAPACITY || radius < 1 || radius > ACCN_MAX_RADIUS || mask_rows < 0 || n_rows < 0 || !counters)
        return PCACC_E_ARG;
    if (!(cos_angle >= 0.0 && cos_angle <= 1.0) || !(max_variation >= 0.0 && max_variation <= 1.0) || !(max_offset >= 0.0)) return PCACC_E_ARG;   // NaN fails
    const void *outs[20] = {out_label, out_distance, out_voxels, out_points, out_lo, out_hi, out_first_row, out_t_first, out_t_last, out_anchor,
                            out_spread, out_shift, out_s1, out_s2, out_normal, out_eigenvalues, out_centroid, out_offset, out_mse, out_flags};
    const size_t width[20] = {4, 8, 4, 8, 12, 12, 4, 4, 4, 12, 8, 4, 24, 48, 24, 24, 24, 8, 8, 1};
    const void *ins[7] = {keys, acc, stamps, normals, eigenvalues, flags, mask};
    const size_t in_bytes[7] = {8 * (size_t)capacity, 8 * ACC_FIELDS * (size_t)capacity, 8 * (size_t)capacity, 12 * (size_t)n_rows, 12 * (size_t)n_rows,
                                (size_t)n_rows, (size_t)mask_rows};
    AcplWs w;
    if (m > 0) {
        if (!keys || !acc || !stamps || !workspace || (mask_rows > 0 && !mask) || (n_rows > 0 && (!normals || !eigenvalues || !flags))) return PCACC_E_ARG;
        for (int a = 0; a < 20; ++a)
            if (!outs[a]) return PCACC_E_ARG;
        if (workspace_bytes < acpl_carve(&w, (char *)workspace, m)) return PCACC_E_ARG;
    }
    for (int b = 0; b < 7; ++b) {
        if (accum_bytes_overlap(counters, ACPL_COUNTERS * sizeof(int64_t), ins[b], in_bytes[b])) return PCACC_E_ARG;
        for (int a = 0; a < 20; ++a)
            if (accum_bytes_overlap(outs[a], width[a] * (size_t)m, ins[b], in_bytes[b])) return PCACC_E_ARG;
    }
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(counters, 0, ACPL_COUNTERS * sizeof(int64_t), st) != hipSuccess) return PCACC_E_LAUNCH;
    if (m == 0) return PCACC_OK;
    if (accn_rows_launch(acc, capacity, m, min_count, (int)use_fraction, max_moving_fraction, w.rows, w.kept, st) != PCACC_OK) return PCACC_E_LAUNCH;
    AcplMap M;
    M.keys = (const unsigned long long *)keys; M.acc = acc; M.stamps = stamps; M.normals = normals; M.eigenvalues = eigenvalues; M.flags = flags;
    M.mask = mask_rows > 0 || mask ? mask : nullptr; M.dst = w.rows.dst; M.rows = w.rows.rows; M.kept = w.kept;
    M.capacity = capacity; M.m = m; M.mask_rows = mask_rows; M.n_rows = n_rows;
    M.cos_angle = cos_angle; M.max_offset = max_offset; M.max_variation = max_variation; M.radius = (int)radius;
    const AcplOut out = {out_label, out_distance, out_voxels, out_points, out_lo, out_hi, out_first_row, out_t_first, out_t_last, out_anchor, out_spread,
                         out_shift, out_s1, out_s2, out_normal, out_eigenvalues, out_centroid, out_offset, out_mse, out_flags,
                         (unsigned long long *)counters};
    const uint8_t *part = w.part;
    const int grid = pcacc_grid(m, ACPL_BLOCK);
    hipLaunchKernelGGL(acpl_class_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, w.parent, w.part, (unsigned long long *)counters);
    // a lane runs up to (2r+1)^2 serial searches: many small workgroups spread over the CUs, as accum_components.hip
    hipLaunchKernelGGL(acpl_link_kernel, dim3(pcacc_grid(m, ACPL_BLOCK, 1 << 22)), dim3(ACPL_BLOCK), 0, st, M, part, w.parent, (unsigned long long *)counters);
    hipLaunchKernelGGL(acpl_flatten_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, w.parent);
    hipLaunchKernelGGL(acpl_root_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, part, (const int *)w.parent, w.flag);
    PCACC_CHECK_LAUNCH();
    pcacc_scan_i32(w.flag, m, w.chunk, w.cid, st);                                                // cid[m] = K
    hipLaunchKernelGGL(acpl_label_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, part, (const int *)w.parent, (const int *)w.cid, out, w.vox64);
    hipLaunchKernelGGL(acpl_stats_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, out, w.vox64);
    hipLaunchKernelGGL(acpl_shift_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, m, out, (const unsigned long long *)w.vox64);
    hipLaunchKernelGGL(acpl_moments_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, out);
    hipLaunchKernelGGL(acpl_fit_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, m, out);
    hipLaunchKernelGGL(acpl_distance_kernel, dim3(grid), dim3(ACPL_BLOCK), 0, st, M, out);
    PCACC_CHECK_LAUNCH();
    return PCACC_OK;
}
