// Host build of pcaccumulation_amd/csrc/accum_pierce.h (tests/test_accumulate_pierce.py): the end points, the eligibility rule, the voxel walk and the
// row lookup of a ray -- the function the kernel of accum_pierce.hip calls -- run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK),
// before anything runs on a GPU.
// The tables stand at their capacity with poison behind row m that no result may depend on and no visit may change.
//   in : i64 n, S, m, capacity, use_stamp, stamp, max_steps, has_moving, has_index, has_pose; f64 voxel_size, margin, max_range (< 0: none);
//        f32 points[n][3]; u8 moving[n]; f64 origins[S][3]; i32 origin_index[n]; f64 pose[16]; i64 keys[m]; i32 stamps[2][m]
//   out: i32 pierced[m]; i64 counters[5] (walked, dropped, skipped, truncated, hits); i64 visits
#include "accum_pierce.h"
#include "accum_host.h"

struct Hit {
    int32_t *pierced;
    int64_t m;
    void operator()(int64_t pos) const { PCACC_BOUND(pos, m); ++pierced[pos]; }
};

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 10);
    const std::vector<double> g = rd<double>(f, 3);
    const int64_t n = h[0], S = h[1], m = h[2], cap = h[3];
    const bool use_stamp = h[4] != 0;
    const int32_t stamp = (int32_t)h[5];
    const int max_steps = (int)h[6];
    const double voxel_size = g[0], margin = g[1], max_range = g[2];
    assert(n >= 0 && S >= 1 && m >= 0 && cap >= m && cap >= 1 && max_steps >= 1 && max_steps <= ACCP_MAX_STEPS && voxel_size > 0.0 && margin >= 0.0);
    const std::vector<float> points = rd<float>(f, 3 * n);
    const std::vector<uint8_t> moving = rd<uint8_t>(f, n);
    const std::vector<double> origins = rd<double>(f, 3 * S);
    const std::vector<int32_t> index = rd<int32_t>(f, n);
    const std::vector<double> pose = rd<double>(f, 16);
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = h[9] ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    // rows past m: a key that would mislead any search that read it, stamps that pass every stamp rule
    const Map map = read_map(f, m, cap, false, Fills{0, 0, 0, -7, 0}, MAP_STAMPS);
    std::vector<int32_t> pierced(cap, 0);
    std::vector<int64_t> counters(5, 0);
    int64_t visits = 0;
    for (int64_t i = m; i < cap; ++i) pierced[i] = POISON_COUNT;
    Hit hit = {pierced.data(), m};
    for (int64_t i = 0; i < n; ++i) {
        const int64_t row = accp_origin_index(h[8] ? (int64_t)index[i] : 0, S);
        if (row >= 0) PCACC_BOUND(row, S);
        const double none[3] = {0.0, 0.0, 0.0};
        const double *origin = row >= 0 ? origins.data() + 3 * row : none;
        const bool mv = h[7] && moving[i];
        const AccpRay r = accp_ray(T, points.data() + 3 * i, origin, row >= 0, mv, voxel_size, margin, max_range >= 0.0, max_range, use_stamp, stamp, max_steps,
                                   map.keys.data(), map.stamps.data(), cap, m, hit);
        assert(r.status == ACCP_WALKED || r.status == ACCP_DROPPED || r.status == ACCP_SKIPPED);
        assert(r.visits >= 0 && r.visits <= max_steps && r.hits >= 0 && r.hits <= r.visits);
        assert(r.status == ACCP_WALKED ? r.visits >= 1 : (r.visits == 0 && !r.truncated));
        assert(!r.truncated || r.visits == max_steps);
        counters[r.status] += 1;
        counters[3] += r.truncated;
        counters[4] += r.hits;
        visits += r.visits;
    }
    for (int64_t i = m; i < cap; ++i) assert(pierced[i] == POISON_COUNT);
    assert(counters[0] + counters[1] + counters[2] == n);
    pierced.resize(m);
    wr(o, pierced);
    wr(o, counters);
    wr1(o, visits);
    close_io(f, o);
    return 0;
}
