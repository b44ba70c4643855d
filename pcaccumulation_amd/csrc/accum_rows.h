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
