// Host build of pcaccumulation_amd/csrc/accum_query.h (tests/test_accumulate_query.py): the whole query -- row table, normals (C5's accum_normal_voxel),
// accq_tables, then accq_point and accq_store per scan point, the functions the kernel of accum_query.hip calls -- run on the CPU with every table index
// assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The map's tables stand at a capacity above m with poison behind row m that no
// result may depend on (a key that would mislead any search that read it, a record that passes every filter); every output column is poison before the
// loop, and every row of every column is asserted written exactly once.
//   in : i64 m, capacity, has_pierced, min_count, use_fraction, has_normals, require_normal, radius, min_neighbors, n_viewpoints, stamp_base, n, has_pose,
//        short_rows (the normal tables are handed over this many rows short: BAD_TABLE); f64 max_moving_fraction, voxel_size, max_distance;
//        a map (see accum_host.h); f64 viewpoints[n_viewpoints][3]; f32 points[n][3]; f64 pose[16] (has_pose)
//   out: i64 counters[7]; i64 V (rows the filter keeps); f32 normals[V][3]; u8 flags[V] (has_normals, else nothing); u8 status[n]; i64 count[n], moving[n];
//        i32 t_first[n], t_last[n], pierced[n], row[n]; f32 nearest[n][3]; f64 distance[n], plane_distance[n]
#include "accum_query.h"
#include "accum_host.h"

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 14);
    const std::vector<double> g = rd<double>(f, 3);
    const int64_t m = h[0], cap = h[1], min_count = h[3], n_view = h[9], stamp_base = h[10], n = h[11], short_rows = h[13];
    const bool has_pierced = h[2] != 0, use_fraction = h[4] != 0, has_normals = h[5] != 0, require_normal = h[6] != 0, has_pose = h[12] != 0;
    const int radius = (int)h[7], min_neighbors = (int)h[8];
    const double frac = g[0], voxel_size = g[1], max_distance = g[2];
    assert(n >= 0 && n_view >= 0 && short_rows >= 0 && (has_normals || !require_normal));
    assert(!has_normals || (radius >= 1 && radius <= ACCN_MAX_RADIUS && min_neighbors >= ACCN_MIN_NEIGHBORS));
    assert(voxel_size > 0.0 && max_distance > 0.0 && max_distance <= voxel_size);
    const Map map = read_map(f, m, cap, has_pierced, Fills{0, 1000, 1000, 0x7fffffff, 77});
    const std::vector<double> view = rd<double>(f, 3 * n_view);
    const std::vector<float> points = rd<float>(f, 3 * n);
    const std::vector<double> pose = rd<double>(f, has_pose ? 16 : 0);
    // the row table (pass 1 of C5) and, when asked for, the normals of the kept rows
    const RowTable tab = row_table(map, min_count, use_fraction, frac);
    const int64_t kept = tab.kept;
    std::vector<float> n32(has_normals ? 3 * kept : 0);
    std::vector<uint8_t> fl(has_normals ? kept : 0);
    for (int64_t j = 0; has_normals && j < kept; ++j) {
        AccnResult r;
        const bool ok = accum_normal_voxel(map.keys.data(), map.acc.data(), map.stamps.data(), cap, m, tab.dst.data(), tab.rows[j], radius, min_neighbors,
                                           n_view > 0 ? view.data() : nullptr, n_view, stamp_base, &r);
        assert(ok);
        for (int a = 0; a < 3; ++a) n32[3 * j + a] = (float)r.normal[a];
        fl[j] = (uint8_t)r.flags;
    }
    // the tables as the caller hands them over: exactly n_rows rows
    const int64_t n_rows = has_normals ? kept - short_rows : 0;
    assert(n_rows >= 0);
    const std::vector<float> n32_given(n32.begin(), n32.begin() + (has_normals ? 3 * n_rows : 0));
    const std::vector<uint8_t> fl_given(fl.begin(), fl.begin() + (has_normals ? n_rows : 0));
    const bool given = has_normals && n_rows > 0;                                         // an empty table is a NULL table
    AccqParams P;
    P.keys = map.keys.data(); P.acc = map.acc.data(); P.stamps = map.stamps.data(); P.pierced = map.p(); P.dst = tab.dst.data();
    P.normals = given ? n32_given.data() : nullptr; P.flags = given ? fl_given.data() : nullptr;
    P.capacity = cap; P.m = m; P.n_rows = n_rows; P.min_count = min_count;
    P.voxel_size = voxel_size; P.max_d2 = max_distance * max_distance; P.max_moving_fraction = frac;
    P.use_fraction = use_fraction; P.require_normal = require_normal && given;
    const int tables = accq_tables(given, m > 0 ? kept : 0, n_rows);
    assert((tables == ACCQ_BAD_TABLES) == (given && short_rows > 0));
    double T[16];
    pcacc_pose_seed(T, has_pose ? pose.data() : nullptr);
    // outputs: poison everywhere
    std::vector<uint8_t> status = poisoned<uint8_t>(n);
    std::vector<int64_t> count = poisoned<int64_t>(n), moving = poisoned<int64_t>(n);
    std::vector<int32_t> t_first = poisoned<int32_t>(n), t_last = poisoned<int32_t>(n), prc = poisoned<int32_t>(n), row = poisoned<int32_t>(n);
    std::vector<float> nearest = poisoned<float>(3 * n);
    std::vector<double> distance = poisoned<double>(n), plane = poisoned<double>(n);
    const AccqOut out = {status.data(), count.data(), moving.data(), t_first.data(), t_last.data(), prc.data(), row.data(), nearest.data(),
                         distance.data(), plane.data()};
    std::vector<int> written(n, 0);
    std::vector<int64_t> counters(ACCQ_COUNTERS, 0);
    for (int64_t i = 0; i < n; ++i) {
        AccqRecord r;
        accq_point(P, tables, T, points.data() + 3 * i, &r);
        assert(is_poison(status[i]) && is_poison(count[i]) && is_poison(moving[i]) && is_poison(t_first[i]) && is_poison(t_last[i]) && is_poison(prc[i]) &&
               is_poison(row[i]) && is_poison(nearest[3 * i]) && is_poison(nearest[3 * i + 1]) && is_poison(nearest[3 * i + 2]) &&
               is_poison(distance[i]) && is_poison(plane[i]));                                   // not written yet
        assert(accq_store(out, i, n, r));
        written[i] += 1;
        assert(r.status >= 0 && r.status < 32 && r.row >= -1 && r.row < kept);
        assert(!(r.status & ACCQ_INVALID) || r.status == ACCQ_INVALID);
        assert(!(r.status & ACCQ_KEPT) || (r.status & ACCQ_OCCUPIED));
        assert(!(r.status & ACCQ_NORMAL) || (r.status & ACCQ_MATCHED));
        assert(((r.status & ACCQ_MATCHED) != 0) == (r.row >= 0));
        counters[ACCQ_C_POINTS] += 1;
        counters[ACCQ_C_INVALID] += (r.status & ACCQ_INVALID) != 0; counters[ACCQ_C_OCCUPIED] += (r.status & ACCQ_OCCUPIED) != 0;
        counters[ACCQ_C_KEPT] += (r.status & ACCQ_KEPT) != 0; counters[ACCQ_C_MATCHED] += (r.status & ACCQ_MATCHED) != 0;
        counters[ACCQ_C_NORMAL] += (r.status & ACCQ_NORMAL) != 0;
    }
    counters[ACCQ_C_BAD_TABLE] = (n > 0 && tables == ACCQ_BAD_TABLES) ? 1 : 0;                   // n = 0 launches nothing: the zero counters
    for (int64_t i = 0; i < n; ++i) {
        assert(written[i] == 1);
        assert(!is_poison(status[i]) && !is_poison(count[i]) && !is_poison(moving[i]) && !is_poison(t_first[i]) && !is_poison(t_last[i]) &&
               !is_poison(prc[i]) && !is_poison(row[i]) && !is_poison(nearest[3 * i]) && !is_poison(nearest[3 * i + 1]) && !is_poison(nearest[3 * i + 2]) &&
               !is_poison(distance[i]) && !is_poison(plane[i]));
        assert(tables != ACCQ_BAD_TABLES || !(status[i] & (ACCQ_MATCHED | ACCQ_NORMAL)));
    }
    wr(o, counters);
    wr1(o, kept);
    wr(o, n32); wr(o, fl);
    wr(o, status); wr(o, count); wr(o, moving); wr(o, t_first); wr(o, t_last); wr(o, prc); wr(o, row); wr(o, nearest); wr(o, distance); wr(o, plane);
    close_io(f, o);
    return 0;
}
