// Host build of pcaccumulation_amd/csrc/accum_raycast.h (tests/test_accumulate_raycast.py): the whole call -- row table, then accy_ray and accy_store per
// ray, the functions the kernel of accum_raycast.hip calls -- run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything
// runs on a GPU.  The map's tables stand at a capacity above m with poison behind row m that no result may depend on (a key that would mislead any search
// that read it, a record that passes every filter); every output column is poison before the loop, and every row of every column is asserted written
// exactly once.
//   in : i64 n, S, m, capacity, max_steps, has_index, has_pose, min_count, use_fraction; f64 voxel_size, min_range, max_range (< 0: none), margin,
//        max_moving_fraction; f32 targets[n][3]; f64 origins[S][3]; i32 origin_index[n] (has_index); f64 pose[16] (has_pose); i64 keys[m]; i64 acc[5][m]
//   out: i64 counters[7]; i64 V (rows the filter keeps); u8 status[n]; i32 row[n], coords[n][3]; f32 point[n][3]; f64 range_in[n], depth[n], length[n];
//        i32 visits[n]
#include "accum_raycast.h"
#include "accum_host.h"

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
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
    // rows past m: a key that would mislead any search that read it, a record that passes every filter (none of its points moving)
    const Map map = read_map(f, m, cap, false, Fills{0, 1000, 0, 0, 0}, MAP_ACC);
    // the row table (pass 1 of C5)
    const RowTable tab = row_table(map, min_count, use_fraction, frac);
    const int64_t kept = tab.kept;
    AccyParams P;
    P.keys = map.keys.data(); P.acc = map.acc.data(); P.dst = tab.dst.data();
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
    wr1(o, kept);
    wr(o, status); wr(o, row); wr(o, coords); wr(o, point); wr(o, range_in); wr(o, depth); wr(o, length); wr(o, visits);
    close_io(f, o);
    return 0;
}
