// Host build of pcaccumulation_amd/csrc/accum_knn.h (tests/test_accumulate_knn.py): the whole search -- row table, then acck_point (scan mode) or acck_row
// (self mode) and acck_store per query, the functions the kernels of accum_knn.hip call -- run on the CPU with every table index assert-checked
// (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The map's tables stand at a capacity above m with poison behind row m that no result may depend
// on (a key that would mislead any search that read it, a record that passes every filter); every output column is poison before the loop, and every
// row of every column is asserted written exactly once.
//   in : i64 m, capacity, min_count, use_fraction, n, has_pose, k, radius, self; f64 max_moving_fraction, voxel_size, max_distance;
//        a map without stamps (see accum_host.h); f32 points[n][3]; f64 pose[16] (has_pose)
//   out: i64 counters[5]; i64 V (rows the filter keeps); i64 R (result rows: n, or V in self mode); i32 rows[R][k]; f64 distance[R][k]; i32 found[R];
//        u8 status[R]; f64 mean_distance[R] (self mode, else nothing)
#include "accum_knn.h"
#include "accum_host.h"

struct Run {
    AcckParams P;
    const RowTable *tab;
    const std::vector<float> *points;
    const double *T;
    int64_t n;
    bool self;
};

template <int K> static void run(const Run &u, FILE *o)
{
    const int k = u.P.k;
    const int64_t kept = u.tab->kept, R = u.self ? kept : u.n;
    std::vector<int32_t> rows = poisoned<int32_t>(R * k), found = poisoned<int32_t>(R);
    std::vector<double> distance = poisoned<double>(R * k), mean = poisoned<double>(u.self ? R : 0);
    std::vector<uint8_t> status = poisoned<uint8_t>(R);
    const AcckOut out = {rows.data(), distance.data(), found.data(), status.data(), u.self ? mean.data() : nullptr};
    std::vector<int> written(R, 0);
    std::vector<int64_t> counters(ACCK_COUNTERS, 0);
    for (int64_t q = 0; q < R; ++q) {
        AcckTop<K> top;
        int st = 0;
        if (u.self) {
            const int64_t i = u.tab->rows[q];
            assert(u.tab->dst[i] == q);
            assert(acck_row(u.P, i, top));
        } else {
            st = acck_point(u.P, u.T, u.points->data() + 3 * q, top);
        }
        assert(st == 0 || st == ACCK_INVALID);
        for (int s = 0; s < K; ++s) {                                                           // ascending in (d2, row), the empty slots last
            assert((top.row[s] >= 0) == (top.d2[s] <= u.P.max_d2) && top.row[s] >= -1 && top.row[s] < kept);
            assert(s == 0 || top.row[s] < 0 || top.d2[s - 1] < top.d2[s] || (top.d2[s - 1] == top.d2[s] && top.row[s - 1] < top.row[s]));
            assert(s == 0 || top.row[s - 1] >= 0 || top.row[s] < 0);
            assert(!u.self || top.row[s] != q);
        }
        assert(is_poison(found[q]) && is_poison(status[q]) && (!u.self || is_poison(mean[q])));  // not written yet
        for (int s = 0; s < k; ++s) assert(is_poison(rows[q * k + s]) && is_poison(distance[q * k + s]));
        const int f = acck_store(out, q, R, k, top, st);
        written[q] += 1;
        assert(f >= 0 && f <= k && found[q] == f && (st == 0 || f == 0));
        assert(status[q] == (st | (f > 0 ? ACCK_FOUND : 0) | (f == k ? ACCK_FULL : 0)));
        counters[ACCK_C_QUERIES] += 1;
        counters[ACCK_C_INVALID] += (st & ACCK_INVALID) != 0;
        counters[ACCK_C_FOUND] += f > 0;
        counters[ACCK_C_FULL] += f == k;
        counters[ACCK_C_NEIGHBORS] += f;
    }
    for (int64_t q = 0; q < R; ++q) {
        assert(written[q] == 1 && !is_poison(found[q]) && !is_poison(status[q]) && (!u.self || !is_poison(mean[q])));
        for (int s = 0; s < k; ++s) {
            assert(!is_poison(rows[q * k + s]) && !is_poison(distance[q * k + s]));
            assert((s < found[q]) == (rows[q * k + s] >= 0));
        }
    }
    wr(o, counters);
    wr1(o, kept);
    wr1(o, R);
    wr(o, rows); wr(o, distance); wr(o, found); wr(o, status); wr(o, mean);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const std::vector<double> g = rd<double>(f, 3);
    const int64_t m = h[0], cap = h[1], min_count = h[2], n = h[4];
    const bool use_fraction = h[3] != 0, has_pose = h[5] != 0, self = h[8] != 0;
    const int k = (int)h[6], radius = (int)h[7];
    const double frac = g[0], voxel_size = g[1], max_distance = g[2];
    assert(n >= 0 && k >= 1 && k <= ACCK_MAX_K && radius >= 1 && radius <= ACCK_MAX_RADIUS && (!self || n == 0));
    assert(voxel_size > 0.0 && max_distance > 0.0 && max_distance <= (double)radius * voxel_size);
    const Map map = read_map(f, m, cap, false, Fills{0, 1000, 1000, 0x7fffffff, 77}, MAP_ACC);
    const std::vector<float> points = rd<float>(f, 3 * n);
    const std::vector<double> pose = rd<double>(f, has_pose ? 16 : 0);
    const RowTable tab = row_table(map, min_count, use_fraction, frac);                         // pass 1 of C5
    double T[16];
    pcacc_pose_seed(T, has_pose ? pose.data() : nullptr);
    Run u;
    u.P.keys = map.keys.data(); u.P.acc = map.acc.data(); u.P.dst = tab.dst.data();
    u.P.capacity = cap; u.P.m = m; u.P.voxel_size = voxel_size; u.P.max_d2 = max_distance * max_distance; u.P.radius = radius; u.P.k = k;
    u.tab = &tab; u.points = &points; u.T = T; u.n = n; u.self = self;
    switch (acck_slots(k)) {
    case 1: run<1>(u, o); break;
    case 2: run<2>(u, o); break;
    case 4: run<4>(u, o); break;
    case 8: run<8>(u, o); break;
    case 16: run<16>(u, o); break;
    default: assert(false);
    }
    close_io(f, o);
    return 0;
}
