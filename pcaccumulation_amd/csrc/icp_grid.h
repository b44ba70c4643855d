// C3. The target index of the ICP refinement (icp.hip): cell / key arithmetic, the hash probe and the 27-cell nearest-neighbour walk as
// __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build (tests/icp_host_driver.cpp) where every table
// index is assert-checked before anything runs on a GPU.  Includes nothing of HIP.
//
// Grid: cells of edge h = the ICP threshold; cell of a coordinate v = floor(v / h) in float64.  A target point is stored iff its three
// coordinates are finite and its cell indices lie in [-32768, 32767]; a query has a correspondence only if its coordinates are finite and its
// cell indices lie in [-32767, 32766] (its 27 neighbour cells are then all representable: nothing is clamped, and a coordinate outside the
// range never forms an address).  Any target within h of a query lies in one of those 27 cells.
// Key: (segment + 1) << 48 | (ix + 32768) << 32 | (iy + 32768) << 16 | (iz + 32768); never 0, so 0 marks an empty slot.  segment < 65535.
// Table: open addressing, linear probing, slots = a power of two >= 2 * (number of points), so it cannot fill up; slot s owns the entries
// list[start[s] .. start[s + 1]) (target point indices, in no particular order: the walk orders candidates by (distance^2, index) itself,
// so equal distances resolve to the lowest target index whatever the order of insertion was).
#pragma once
#include "hd.h"

#define ICP_CELL_MIN (-32768)
#define ICP_CELL_MAX 32767
#define ICP_MAX_SEGMENTS 65535

struct IcpGrid {
    const unsigned long long *keys;   // [slots]
    const int32_t *start;             // [slots + 1]
    const int32_t *list;              // [n_list]
    const float *points;              // [n, 3]
    uint32_t mask;                    // slots - 1
    int64_t n, n_list;
    double h;                         // cell edge
};

// Cell index of v, valid only when the function returns true: v is finite and floor(v / h) lies in [lo, hi].
PCACC_HD bool icp_cell(double v, double h, int lo, int hi, int *cell)
{
    if (!pcacc_finite(v)) return false;
    const double c = __builtin_floor(v / h);
    if (!(c >= (double)lo && c <= (double)hi)) return false;           // also false when v / h overflowed
    *cell = (int)c;
    return true;
}

PCACC_HD bool icp_target_cell(const double p[3], double h, int c[3])
{
    return icp_cell(p[0], h, ICP_CELL_MIN, ICP_CELL_MAX, &c[0]) && icp_cell(p[1], h, ICP_CELL_MIN, ICP_CELL_MAX, &c[1]) &&
           icp_cell(p[2], h, ICP_CELL_MIN, ICP_CELL_MAX, &c[2]);
}

PCACC_HD bool icp_query_cell(const double p[3], double h, int c[3])
{
    return icp_cell(p[0], h, ICP_CELL_MIN + 1, ICP_CELL_MAX - 1, &c[0]) && icp_cell(p[1], h, ICP_CELL_MIN + 1, ICP_CELL_MAX - 1, &c[1]) &&
           icp_cell(p[2], h, ICP_CELL_MIN + 1, ICP_CELL_MAX - 1, &c[2]);
}

// seg in [0, ICP_MAX_SEGMENTS), cell indices in [ICP_CELL_MIN, ICP_CELL_MAX]
PCACC_HD unsigned long long icp_key(int seg, int ix, int iy, int iz)
{
    return ((unsigned long long)(seg + 1) << 48) | ((unsigned long long)(ix - ICP_CELL_MIN) << 32) |
           ((unsigned long long)(iy - ICP_CELL_MIN) << 16) | (unsigned long long)(iz - ICP_CELL_MIN);
}

PCACC_HD uint32_t icp_hash(unsigned long long x, uint32_t mask)         // the 64-bit finaliser of MurmurHash3
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t)x & mask;
}

// The segment that holds point i -- the last s with offsets[s] <= i, which skips empty segments -- or -1.  offsets [n_seg + 1] ascending.
PCACC_HD int icp_segment_of(const int32_t *offsets, int n_seg, int64_t i)
{
    PCACC_BOUND(n_seg, n_seg + 1);
    if (i < offsets[0] || i >= offsets[n_seg]) return -1;
    int lo = 0, hi = n_seg;                                   // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        PCACC_BOUND(mid, n_seg + 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Slot of `key`, or -1 when the table does not hold it.  Read-only; at most mask + 1 probes.
PCACC_HD int64_t icp_find(const unsigned long long *keys, uint32_t mask, unsigned long long key)
{
    uint32_t s = icp_hash(key, mask);
    for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {
        PCACC_BOUND(s, (int64_t)mask + 1);
        const unsigned long long k = keys[s];
        if (k == key) return s;
        if (k == 0) return -1;
    }
    return -1;
}

// Nearest point of segment `seg` to q among the 27 cells around q: index into g.points or -1; *d2_out its squared distance.
// A candidate counts iff d2 <= thr2; of equal d2 the lowest index wins.  float64 throughout, the fp32 coordinates promoted.
PCACC_HD int64_t icp_nearest(const IcpGrid &g, int seg, const double q[3], double thr2, double *d2_out)
{
    PCACC_NO_CONTRACT
    int c[3];
    if (!icp_query_cell(q, g.h, c)) return -1;
    int64_t best = -1;
    double best_d2 = 0.0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int64_t s = icp_find(g.keys, g.mask, icp_key(seg, c[0] + dx, c[1] + dy, c[2] + dz));
                if (s < 0) continue;
                PCACC_BOUND(s + 1, (int64_t)g.mask + 2);
                const int32_t lo = g.start[s], hi = g.start[s + 1];
                for (int32_t e = lo; e < hi; ++e) {
                    PCACC_BOUND(e, g.n_list);
                    const int64_t i = g.list[e];
                    PCACC_BOUND(i, g.n);
                    const double ex = (double)g.points[3 * i] - q[0], ey = (double)g.points[3 * i + 1] - q[1],
                                 ez = (double)g.points[3 * i + 2] - q[2];
                    const double d2 = ex * ex + ey * ey + ez * ez;
                    if (!(d2 <= thr2)) continue;
                    if (best < 0 || d2 < best_d2 || (d2 == best_d2 && i < best)) { best = i; best_d2 = d2; }
                }
            }
    *d2_out = best_d2;
    return best;
}

// R p + t of a row-major 4x4 (the last row is taken as 0 0 0 1), float64.
PCACC_HD void icp_apply(const double *T, const float *p, double q[3])
{
    PCACC_NO_CONTRACT
    const double x = p[0], y = p[1], z = p[2];
    q[0] = T[0] * x + T[1] * y + T[2] * z + T[3];
    q[1] = T[4] * x + T[5] * y + T[6] * z + T[7];
    q[2] = T[8] * x + T[9] * y + T[10] * z + T[11];
}
