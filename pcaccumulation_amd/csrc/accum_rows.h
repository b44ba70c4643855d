// Pass 1 of C5 (accum_normals.hip defines it; accum_register.hip calls it): keep flags (extract's predicate) -> scan.h -> dst[m], the output row of every
// map row (-1 = does not participate), rows[kept] its inverse, kpos[m] = kept.  One launch sequence for both callers: the row table of a registration
// is the row table of the normals it reads.
#pragma once
#include "common.h"

struct AccnRows { int *dst, *kpos, *rows, *chunk; };

// The four tables carved from `base` (NULL: sizes only); -> bytes taken.
size_t accn_rows_carve(int64_t m, AccnRows *t, char *base);
// m >= 1.  *out_n = kept (device).  PCACC_OK or PCACC_E_LAUNCH.
int accn_rows_launch(const int64_t *acc, int64_t capacity, int64_t m, int64_t min_count, int use_fraction, double max_moving_fraction, const AccnRows &t,
                     int64_t *out_n, hipStream_t st);

// The row table and the kept word that accn_rows_launch leaves on the device: the head of the workspace of C9, C10 and C11.
struct AccnRowsWs { AccnRows rows; int64_t *kept; };

// m = 0 carves as m = 1.  -> bytes taken; the caller's own tables follow at base + that.
static inline size_t accn_rows_ws_carve(int64_t m, AccnRowsWs *w, char *base)
{
    const size_t off = accn_rows_carve(m > 0 ? m : 1, &w->rows, base);
    w->kept = (int64_t *)(base + off);
    return off + pcacc_align(sizeof(int64_t));
}
