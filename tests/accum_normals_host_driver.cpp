// Host build of pcaccumulation_amd/csrc/accum_normals.h (tests/test_accumulate_normals.py): the offset / range test, the neighbour row search and the
// whole result of a voxel -- the function the kernel of accum_normals.hip calls -- run on the CPU with every table index assert-checked
// (-DPCACC_HOST_CHECK), before anything runs on a GPU.  Pass 1 (keep flags, scan, dst / rows tables) is accum_host.h's row table.
//   in : i64 m, capacity, min_count, use_fraction, radius, min_neighbors, n_viewpoints, stamp_base; f64 max_moving_fraction;
//        a map without a sidecar (see accum_host.h); f64 viewpoints[n_viewpoints][3]
//   out: i64 V; f64 normals[V][3]; f64 eigenvalues[V][3]; i32 neighbors[V]; u8 flags[V]; f32 normals[V][3]; f32 eigenvalues[V][3]
#include "accum_normals.h"
#include "accum_host.h"

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 8);
    const double frac = rd<double>(f, 1)[0];
    const int64_t m = h[0], cap = h[1], min_count = h[2], n_view = h[6], stamp_base = h[7];
    const bool use_fraction = h[3] != 0;
    const int radius = (int)h[4], min_neighbors = (int)h[5];
    assert(radius >= 1 && radius <= ACCN_MAX_RADIUS && min_neighbors >= ACCN_MIN_NEIGHBORS && n_view >= 0);
    // the tables at their capacity: rows past m hold a pattern no result may depend on
    const Map map = read_map(f, m, cap, false, Fills{ACC_INVALID_KEY, -7, -7, -7, 0});
    const std::vector<double> view = rd<double>(f, 3 * n_view);
    // pass 1
    const RowTable t = row_table(map, min_count, use_fraction, frac);
    const int64_t kept = t.kept;
    // pass 2
    std::vector<double> n64(3 * kept), e64(3 * kept);
    std::vector<float> n32(3 * kept), e32(3 * kept);
    std::vector<int32_t> nb(kept);
    std::vector<uint8_t> fl(kept);
    for (int64_t j = 0; j < kept; ++j) {
        const int64_t i = t.rows[j];
        assert(i >= 0 && i < m && t.dst[i] == j);
        AccnResult r;
        const bool ok = accum_normal_voxel(map.keys.data(), map.acc.data(), map.stamps.data(), cap, m, t.dst.data(), i, radius, min_neighbors,
                                           n_view > 0 ? view.data() : nullptr, n_view, stamp_base, &r);
        assert(ok);
        assert(r.k >= 1 && r.k <= (2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1));
        for (int a = 0; a < 3; ++a) {
            n64[3 * j + a] = r.normal[a]; e64[3 * j + a] = r.s[a];
            n32[3 * j + a] = (float)r.normal[a]; e32[3 * j + a] = (float)r.s[a];
        }
        nb[j] = r.k;
        fl[j] = (uint8_t)r.flags;
    }
    wr1(o, kept);
    wr(o, n64); wr(o, e64); wr(o, nb); wr(o, fl); wr(o, n32); wr(o, e32);
    close_io(f, o);
    return 0;
}
