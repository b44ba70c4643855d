// C14. Observed space: the voxels that measured rays crossed (accum_observe.hip; include/pcacc.h C14): the walk of one ray with
// its visits handed to the caller, the index arithmetic of the route (runs, search, decisions, merge) and the lookup of one row as __host__ __device__
// functions, so that the SAME code runs in the kernels and in a g++ build (tests/accum_observe_host_driver.cpp) where every table index is
// assert-checked before anything runs on a GPU.  Includes nothing of HIP.  Float64 appears only in the walk (+, -, *, / and sqrt, no FMA contraction).
//
// A ray is C7's ray (accum_pierce.h), bit for bit, up to the visit: end points, drop rule, "moving is SKIPPED", t_end with margin and max_range, the walk
// by accp_step, max_steps and the TRUNCATED rule.  Every visited voxel contributes its key -- the start voxel included, whether or not any cloud keeps
// the voxel.  The walk is monotone on every axis: one ray visits a voxel at most once.
// The loop of accp_ray is written out once more in acco_walk: moving it into a helper that both call changed the register count the compiler gives
// accp_pierce_kernel (section 9n has the figures).  The host driver asserts that the two visit sequences are equal on every scene.
//
// The table: keys [capacity] ascending and duplicate-free (accum_key), rays [capacity] i64, stamps [2][capacity] i32 (t_first, t_last).
//   rays[v]    = walked rays, over all calls, whose walk visited v
//   t_first[v] = min, t_last[v] = max of the stamp of the calls in which some ray visited v
// All integers: the table is a function of the SET of (ray, stamp) pairs.
#pragma once
#include "accum_pierce.h"

#if defined(__HIPCC__)
#define ACCO_MEMBER __host__ __device__ __forceinline__
#else
#define ACCO_MEMBER inline
#endif

// status of a call, in its state word (include/pcacc.h mirrors the values; accum_observe.hip static_asserts that)
#define ACCO_OK 0
#define ACCO_TOO_SMALL 1                // the merged table has more rows than the output tables
#define ACCO_BAD_STATE 2                // the state words do not describe the input tables
#define ACCO_TOO_MANY 3                 // the rays of the call make more visits than visit_capacity
// status bits of a looked-up row
#define ACCO_VALID 1
#define ACCO_SEEN 2
#define ACCO_ENOUGH 4
#define ACCO_MAX_VISITS 2147483648ll    // n * max_steps stays below it: the visit offsets are an int32 scan

struct AccoWalk {
    int status;             // ACCP_WALKED / ACCP_DROPPED / ACCP_SKIPPED
    int truncated;          // 1: cut at max_steps visits
    int visits;             // voxels visited
};

// A visit that only counts (step 1 of the route): the walk counts for it.
struct AccoCount {
    ACCO_MEMBER void operator()(unsigned long long) const {}
};

// A visit that writes its key (step 4): the ray's slots are [at, end) of out, and a visit past them writes nothing.
struct AccoEmit {
    unsigned long long *out;
    int64_t at, end;
    ACCO_MEMBER void operator()(unsigned long long key)
    {
        if (at < end) { PCACC_BOUND(at, end); out[at] = key; }
        ++at;
    }
};

// The whole of one ray.  T: 12 doubles of the pose; p: the scan point; origin: its row of the origin table, read only when origin_ok (origin_index in range);
// t_end's max_range is used when use_range.  visit(key) is called for every visited voxel, in walking order.
template <class Visit>
PCACC_HD AccoWalk acco_walk(const double *T, const float *p, const double *origin, bool origin_ok, bool moving, double voxel_size, double margin, bool use_range,
                            double max_range, int max_steps, Visit &visit)
{
    PCACC_NO_CONTRACT
    AccoWalk r;
    r.status = ACCP_DROPPED; r.truncated = 0; r.visits = 0;
    double e[3], o[3];
    int64_t ie[3], i[3];
    if (!origin_ok) return r;
    if (!accp_end_point(T, origin[0], origin[1], origin[2], voxel_size, o, i)) return r;
    if (!accp_end_point(T, (double)p[0], (double)p[1], (double)p[2], voxel_size, e, ie)) return r;
    r.status = ACCP_SKIPPED;
    if (moving) return r;
    const double dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
    const double L = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(L > 0.0)) return r;
    double t_end = 1.0 - margin / L;
    if (use_range) {
        const double t_range = max_range / L;
        if (t_range < t_end) t_end = t_range;
    }
    if (!(t_end > 0.0)) return r;
    r.status = ACCP_WALKED;
    const double d[3] = {dx, dy, dz};
    double t_in = 0.0;
    for (;;) {
        visit(accum_key(i[0], i[1], i[2]));
        ++r.visits;
        if (!accp_step(o, d, voxel_size, t_end, i, &t_in)) break;
        if (r.visits >= max_steps) { r.truncated = 1; break; }
    }
    return r;
}

// n rays of at most max_steps visits each fit the int32 scan of the visit counts.
PCACC_HD bool acco_visits_fit(int64_t n, int64_t max_steps) { return n >= 0 && max_steps >= 1 && n * max_steps < ACCO_MAX_VISITS; }

// Slots [*at, *end) of ray i in the emitted key list, from the exclusive scan of the visit counts (offsets has n + 1 entries, offsets[n] = V);
// false = the numbers do not fit the list and nothing is addressed.
PCACC_HD bool acco_slots(const int *offsets, int64_t i, int64_t n, int64_t V, int64_t *at, int64_t *end)
{
    PCACC_BOUND(i, n);
    const int64_t a = offsets[i], b = offsets[i + 1];
    if (a < 0 || b < a || b > V) return false;
    *at = a; *end = b;
    return true;
}

// Step 3: the visits of the call against the room for them.
PCACC_HD int acco_decide_visits(bool bad_state, int64_t V, int64_t visit_capacity)
{
    if (bad_state) return ACCO_BAD_STATE;
    return (V < 0 || V > visit_capacity) ? ACCO_TOO_MANY : ACCO_OK;
}

// Step 5: sorted position i of V starts a run (= a voxel of this call).
PCACC_HD int acco_head(const unsigned long long *sorted, int64_t i, int64_t V)
{
    if (i >= V) return 0;
    PCACC_BOUND(i, V);
    return (i == 0 || sorted[i - 1] != sorted[i]) ? 1 : 0;
}

// Rays of run r of R: start has R + 1 entries, start[R] = V.  0 when the numbers do not fit.
PCACC_HD int64_t acco_run_length(const int *start, int64_t r, int64_t R)
{
    PCACC_BOUND(r, R);
    const int64_t len = (int64_t)start[r + 1] - (int64_t)start[r];
    return len > 0 ? len : 0;
}

// Step 6: run key against the first m rows of the table -> its insertion position in [0, m]; *miss = the table does not hold it.
PCACC_HD int64_t acco_search(const unsigned long long *keys, int64_t m, unsigned long long key, int *miss)
{
    const int64_t p = accum_lower_bound(keys, m, key);
    if (p < m) PCACC_BOUND(p, m);
    *miss = !(p < m && keys[p] == key);
    return p;
}

PCACC_HD int acco_decide_rows(int64_t total, int64_t out_capacity) { return total > out_capacity ? ACCO_TOO_SMALL : ACCO_OK; }

// Step 7a: old row p of m goes to p + (misses below it), with the run added where the call holds its key.  mrank: exclusive scan of the miss flags, at
// least R + 1 entries.  -> the destination row, or -1 when nothing was written.
PCACC_HD int64_t acco_merge_old(int64_t p, const unsigned long long *in_keys, const int64_t *in_rays, const int32_t *in_stamps, int64_t in_capacity, int64_t m,
                                const unsigned long long *run_key, const int *run_start, int64_t R, const int *mrank, int64_t total, int32_t stamp,
                                unsigned long long *out_keys, int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity)
{
    PCACC_BOUND(p, m);
    PCACC_BOUND(p, in_capacity);
    const unsigned long long key = in_keys[p];
    const int64_t j = accum_lower_bound(run_key, R, key);                        // in [0, R]
    PCACC_BOUND(j, R + 1);
    const int64_t d = accum_merge_dst(p, mrank[j], total);
    if (d < 0 || d >= out_capacity) return -1;
    PCACC_BOUND(d, out_capacity);
    const bool hit = j < R && run_key[j] == key;
    const int32_t t0 = in_stamps[p], t1 = in_stamps[in_capacity + p];
    out_keys[d] = key;
    out_rays[d] = in_rays[p] + (hit ? acco_run_length(run_start, j, R) : 0);
    out_stamps[d] = (hit && stamp < t0) ? stamp : t0;
    out_stamps[out_capacity + d] = (hit && stamp > t1) ? stamp : t1;
    return d;
}

// Step 7b: run j of R that the table did not hold goes to position + rank.  -> the destination row, or -1 when nothing was written.
PCACC_HD int64_t acco_merge_new(int64_t j, const unsigned long long *run_key, const int *run_start, int64_t R, const int *miss, const int *pos, const int *mrank,
                                int64_t total, int32_t stamp, unsigned long long *out_keys, int64_t *out_rays, int32_t *out_stamps, int64_t out_capacity)
{
    PCACC_BOUND(j, R);
    if (!miss[j]) return -1;
    const int64_t d = accum_merge_dst(pos[j], mrank[j], total);
    if (d < 0 || d >= out_capacity) return -1;
    PCACC_BOUND(d, out_capacity);
    out_keys[d] = run_key[j];
    out_rays[d] = acco_run_length(run_start, j, R);
    out_stamps[d] = stamp;
    out_stamps[out_capacity + d] = stamp;
    return d;
}

// A row of voxel indices: valid iff every index lies in [-2^20, 2^20); the key only then.
PCACC_HD bool acco_coord_key(const int32_t *c, unsigned long long *key)
{
    if (!accp_in_range(c[0]) || !accp_in_range(c[1]) || !accp_in_range(c[2])) return false;
    *key = accum_key(c[0], c[1], c[2]);
    return true;
}

// The lookup of one row: the status bits and the record (0 where unseen or invalid).  m > capacity addresses nothing.
PCACC_HD int acco_lookup(bool valid, unsigned long long key, const unsigned long long *keys, const int64_t *rays, const int32_t *stamps, int64_t capacity,
                         int64_t m, int64_t min_rays, int64_t *out_rays, int32_t *out_first, int32_t *out_last)
{
    *out_rays = 0; *out_first = 0; *out_last = 0;
    if (!valid) return 0;
    int status = ACCO_VALID;
    if (m < 0 || m > capacity) return status;
    const int64_t pos = accum_lower_bound(keys, m, key);                         // in [0, m]; m = 0: no load
    if (pos < m) {
        PCACC_BOUND(pos, m);
        if (keys[pos] == key) {
            status |= ACCO_SEEN;
            *out_rays = rays[pos]; *out_first = stamps[pos]; *out_last = stamps[capacity + pos];
            if (rays[pos] >= min_rays) status |= ACCO_ENOUGH;
        }
    }
    return status;
}
