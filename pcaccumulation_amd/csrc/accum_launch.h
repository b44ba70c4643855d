// What the launchers of the accumulated scene cloud (accum.hip, accum_*.hip) share: the launcher-side counterpart of hd.h.
// HIP only: no contract header and no host driver includes it.  One definition of each piece; a new row takes its scaffolding from here, from
// pcacc_scan_i32 of scan.h and from accn_rows_ws_carve of accum_rows.h.
#pragma once
#include "common.h"
#include "accum_grid.h"

#define ACCUM_MAX_CAPACITY ((int64_t)1 << 30)       // rows of a map: int scans and int row numbers
#define ACCUM_KEEP_BLOCK 256

static __device__ __forceinline__ long long accum_wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Every lane of the wave calls it: v summed over the wave, then one integer atomic per wave, and none for a sum of zero.
static __device__ __forceinline__ void accum_wave_count(unsigned long long *counters, int slot, long long v)
{
    v = accum_wave_sum(v);
    if (lane_id() == 0 && v) atomicAdd(&counters[slot], (unsigned long long)v);
}

// The segmented sum over the 64 lanes of a wave (K4 of add, the reduction of regrid): lane's v plus the v of the lanes before it with the same run r.
static __device__ __forceinline__ long long acc_seg_scan(long long v, int r, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, d, 64);
        const int rr = __shfl_up(r, d, 64);
        if (lane >= d && rr == r) v += t;                       // r ascends along the lanes: equal at distance d = equal all the way
    }
    return v;
}

// Extract's predicate over the first m rows: pcacc_accum_extract and accn_rows_launch (pass 1 of C5) launch it.
static __global__ __launch_bounds__(ACCUM_KEEP_BLOCK) void accum_keep_kernel(const int64_t *__restrict__ acc, int64_t capacity, int64_t m, int64_t min_count,
                                                                              int use_fraction, double max_moving_fraction, int *__restrict__ keep)
{
    for (int64_t i = (int64_t)blockIdx.x * ACCUM_KEEP_BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * ACCUM_KEEP_BLOCK)
        keep[i] = accum_keep(acc[accum_field(0, i, capacity)], acc[accum_field(1, i, capacity)], min_count, use_fraction != 0, max_moving_fraction) ? 1 : 0;
}

// [a, a + na) and [b, b + nb) share a byte; a NULL table shares nothing.
static inline bool accum_bytes_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// An out-of-place launch (prune, remove_components): some input table shares a byte with some output table.
static inline bool accum_tables_overlap(const void *in_keys, const void *in_acc, const void *in_stamps, const void *in_pierced, int64_t in_capacity,
                                        const void *out_keys, const void *out_acc, const void *out_stamps, const void *out_pierced, int64_t out_capacity)
{
    const void *in_tab[4] = {in_keys, in_acc, in_stamps, in_pierced};
    const void *out_tab[4] = {out_keys, out_acc, out_stamps, out_pierced};
    const size_t row_bytes[4] = {8, 8 * ACC_FIELDS, 4 * 2, 4};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            if (accum_bytes_overlap(in_tab[a], row_bytes[a] * (size_t)in_capacity, out_tab[b], row_bytes[b] * (size_t)out_capacity)) return true;
    return false;
}
