// Host build of pcaccumulation_amd/csrc/accum_raycast.h (tests/test_accumulate_raycast.py): the whole call -- row table, then accy_ray and accy_store per
// ray, the functions the kernel of accum_raycast.hip calls -- run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything
// runs on a GPU.  The map's tables stand at a capacity above m with poison behind row m that no result may depend on (a key that would mislead any search
// that read it, a record that passes every filter); every output column is poison before the loop, and every row of every column is asserted written
// exactly once.
//   in : i64 n, S, m, capacity, max_steps, has_index, has_pose, min_count, use_fraction; f64 voxel_size, min_range, max_range (< 0: none), margin,
//        max_moving_fraction; f32 targets[n][3]; f64 origins[S][3]; i32 origin_index[n] (has_index); f64 pose[16] (has_pose); i64 keys[m]; i64 acc[5][m]
//   out: i64 counters[7]; i64 V (rows the filter keeps); u8 status[n]; i32 row[n], coords[n][3]; f32 point[n][3]; f64 range_in[n], depth[n], length[n];
//        i32 visits[n]
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "accum_raycast.h"

typedef unsigned long long u64;

#define POISON_U8 0xa5                  // every byte of every output before the loop

template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n) assert(fread(v.data(), sizeof(T), n, f) == n);
    return v;
}

template <class T> static void wr(FILE *f, const std::vector<T> &v)
{
    if (!v.empty()) assert(fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
}

template <class T> static bool is_poison(const T &v)
{
    unsigned char b[sizeof(T)];
    memcpy(b, &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); ++k)
        if (b[k] != POISON_U8) return false;
    return true;
}

template <class T> static std::vector<T> poisoned(size_t n)
{
    std::vector<T> v(n);
    if (n) memset(v.data(), POISON_U8, n * sizeof(T));
    return v;
}

int main(int argc, char **argv)
{
    assert(argc == 3);
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    assert(f && o);
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const std::vector<double> g = rd<double>(f, 5);
    const int64_t n = h[0], S = h[1], m = h[2], cap = h[3], min_count = h[7];
    const int max_steps = (int)h[4];
    const bool has_index = h[5] != 0, has_pose = h[6] != 0, use_fraction = h[8] != 0;
    const double voxel_size = g[0], min_range = g[1], max_range = g[2], margin = g[3], frac = g[4];
    assert(n >= 0 && S >= 1 && m >= 0 && cap >= m && cap >= 1 && max_steps >= 1 && max_steps <= ACCY_MAX_STEPS);
    assert(voxel_size > 0.0 && min_range >= 0.0 && margin >= 0.0 && max_range == max_range);
    const std::vector<float> targets = rd<float>(f, 3 * n);
    const std::vector<double> origins = rd<double>(f, 3 * S);
    const std::vector<int32_t> index = rd<int32_t>(f, has_index ? n : 0);
    const std::vector<double> pose = rd<double>(f, has_pose ? 16 : 0);
    // rows past m: a key that would mislead any search that read it, a record that passes every filter
    std::vector<u64> keys(cap, 0);
    std::vector<int64_t> acc((size_t)ACC_FIELDS * cap, 1000);
    for (int64_t i = m; i < cap; ++i) acc[accum_field(1, i, cap)] = 0;
    {
        const std::vector<int64_t> k = rd<int64_t>(f, m), a = rd<int64_t>(f, (size_t)ACC_FIELDS * m);
        for (int64_t i = 0; i < m; ++i) {
            keys[i] = (u64)k[i];
            assert(i == 0 || keys[i - 1] < keys[i]);
            for (int c = 0; c < ACC_FIELDS; ++c) acc[(size_t)c * cap + i] = a[(size_t)c * m + i];
        }
    }
    // the row table (pass 1 of C5)
    std::vector<int> dst(m), kpos(m + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        dst[i] = accum_keep(acc[accum_field(0, i, cap)], acc[accum_field(1, i, cap)], min_count, use_fraction, frac) ? 1 : 0;
        kpos[i + 1] = kpos[i] + dst[i];
    }
    const int64_t kept = kpos[m];
    for (int64_t i = 0; i < m; ++i) {
        const int64_t d = dst[i] ? accum_merge_dst(kpos[i], 0, kept) : -1;
        assert(!dst[i] || d >= 0);
        dst[i] = (int)d;
    }
    AccyParams P;
    P.keys = keys.data(); P.acc = acc.data(); P.dst = dst.data();
    P.capacity = cap; P.m = m;
    P.voxel_size = voxel_size; P.min_range = min_range; P.margin = margin; P.max_range = max_range;
    P.use_range = max_range >= 0.0 ? 1 : 0; P.max_steps = max_steps;
    double T[16];
    pcacc_pose_seed(T, has_pose ? pose.data() : nullptr);
    // outputs: poison everywhere
    std::vector<uint8_t> status = poisoned<uint8_t>(n);
    std::vector<int32_t> row = poisoned<int32_t>(n), coords = poisoned<int32_t>(3 * n), visits = poisoned<int32_t>(n);
    std::vector<float> point = poisoned<float>(3 * n);
    std::vector<double> range_in = poisoned<double>(n), depth = poisoned<double>(n), length = poisoned<double>(n);
    const AccyOut out = {status.data(), row.data(), coords.data(), point.data(), range_in.data(), depth.data(), length.data(), visits.data()};
    std::vector<int> written(n, 0);
    std::vector<int64_t> counters(ACCY_COUNTERS, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t orow = accp_origin_index(has_index ? (int64_t)index[i] : 0, S);
        if (orow >= 0) PCACC_BOUND(orow, S);
        const double none[3] = {0.0, 0.0, 0.0};
        const double *origin = orow >= 0 ? origins.data() + 3 * orow : none;
        AccyRecord r;
        accy_ray(P, T, targets.data() + 3 * i, origin, orow >= 0, &r);
        bool fresh = is_poison(status[i]) && is_poison(row[i]) && is_poison(visits[i]) && is_poison(range_in[i]) && is_poison(depth[i]) && is_poison(length[i]);
        for (int a = 0; a < 3; ++a) fresh = fresh && is_poison(coords[3 * i + a]) && is_poison(point[3 * i + a]);
        assert(fresh);                                                                            // not written yet
        assert(accy_store(out, i, n, r));
        written[i] += 1;
        assert(r.status >= ACCY_MISS && r.status <= ACCY_DROPPED && r.visits >= 0 && r.visits <= max_steps && r.row >= -1 && r.row < kept);
        assert((r.status == ACCY_HIT) == (r.row >= 0));
        assert((r.status == ACCY_SKIPPED || r.status == ACCY_DROPPED) == (r.visits == 0));
        assert(r.status != ACCY_TRUNCATED || r.visits == max_steps);
        assert(r.status != ACCY_DROPPED || r.length == 0.0);
        assert(r.status == ACCY_HIT || (r.range_in == __builtin_inf() && r.depth == __builtin_inf() && r.coord_x == 0 && r.coord_y == 0 && r.coord_z == 0 &&
                                       r.point_x == 0.0f && r.point_y == 0.0f && r.point_z == 0.0f));
        counters[ACCY_C_RAYS] += 1;
        counters[ACCY_C_DROPPED] += r.status == ACCY_DROPPED; counters[ACCY_C_SKIPPED] += r.status == ACCY_SKIPPED; counters[ACCY_C_HIT] += r.status == ACCY_HIT;
        counters[ACCY_C_MISSED] += r.status == ACCY_MISS; counters[ACCY_C_TRUNCATED] += r.status == ACCY_TRUNCATED; counters[ACCY_C_VISITS] += r.visits;
    }
    for (int64_t i = 0; i < n; ++i) {
        assert(written[i] == 1);
        bool all = !is_poison(status[i]) && !is_poison(row[i]) && !is_poison(visits[i]) && !is_poison(range_in[i]) && !is_poison(depth[i]) && !is_poison(length[i]);
        for (int a = 0; a < 3; ++a) all = all && !is_poison(coords[3 * i + a]) && !is_poison(point[3 * i + a]);
        assert(all);
    }
    assert(counters[ACCY_C_RAYS] == n && counters[ACCY_C_DROPPED] + counters[ACCY_C_SKIPPED] + counters[ACCY_C_HIT] + counters[ACCY_C_MISSED] +
                                                counters[ACCY_C_TRUNCATED] == n);
    wr(o, counters);
    assert(fwrite(&kept, 8, 1, o) == 1);
    wr(o, status); wr(o, row); wr(o, coords); wr(o, point); wr(o, range_in); wr(o, depth); wr(o, length); wr(o, visits);
    fclose(o);
    fclose(f);
    return 0;
}
