// Host build of pcaccumulation_amd/csrc/accum_normals.h (tests/test_accumulate_normals.py): the offset / range test, the neighbour row search and the
// whole result of a voxel -- the function the kernel of accum_normals.hip calls -- run on the CPU with every table index assert-checked
// (-DPCACC_HOST_CHECK), before anything runs on a GPU.  Pass 1 (keep flags, scan, dst / rows tables) is restated here with the same helpers.
//   in : i64 m, capacity, min_count, use_fraction, radius, min_neighbors, n_viewpoints, stamp_base; f64 max_moving_fraction;
//        i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; f64 viewpoints[n_viewpoints][3]
//   out: i64 V; f64 normals[V][3]; f64 eigenvalues[V][3]; i32 neighbors[V]; u8 flags[V]; f32 normals[V][3]; f32 eigenvalues[V][3]
#include <cassert>
#include <cstdio>
#include <vector>

#include "accum_normals.h"

typedef unsigned long long u64;

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

int main(int argc, char **argv)
{
    assert(argc == 3);
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    assert(f && o);
    const std::vector<int64_t> h = rd<int64_t>(f, 8);
    const double frac = rd<double>(f, 1)[0];
    const int64_t m = h[0], cap = h[1], min_count = h[2], n_view = h[6], stamp_base = h[7];
    const bool use_fraction = h[3] != 0;
    const int radius = (int)h[4], min_neighbors = (int)h[5];
    assert(m >= 0 && cap >= m && cap >= 1 && radius >= 1 && radius <= ACCN_MAX_RADIUS && min_neighbors >= ACCN_MIN_NEIGHBORS && n_view >= 0);
    // the tables at their capacity: rows past m hold a pattern no result may depend on
    std::vector<u64> keys(cap, ACC_INVALID_KEY);
    std::vector<int64_t> acc(ACC_FIELDS * cap, -7);
    std::vector<int32_t> stamps(2 * cap, -7);
    {
        const std::vector<int64_t> k = rd<int64_t>(f, m), a = rd<int64_t>(f, ACC_FIELDS * m);
        const std::vector<int32_t> s = rd<int32_t>(f, 2 * m);
        for (int64_t i = 0; i < m; ++i) {
            keys[i] = (u64)k[i];
            assert(i == 0 || keys[i - 1] < keys[i]);
            for (int fl = 0; fl < ACC_FIELDS; ++fl) acc[accum_field(fl, i, cap)] = a[fl * m + i];
            stamps[i] = s[i];
            stamps[cap + i] = s[m + i];
        }
    }
    const std::vector<double> view = rd<double>(f, 3 * n_view);
    // pass 1
    std::vector<int> dst(m), kpos(m + 1, 0), rows(m, -1);
    for (int64_t i = 0; i < m; ++i) {
        dst[i] = accum_keep(acc[accum_field(0, i, cap)], acc[accum_field(1, i, cap)], min_count, use_fraction, frac) ? 1 : 0;
        kpos[i + 1] = kpos[i] + dst[i];
    }
    const int64_t kept = kpos[m];
    for (int64_t i = 0; i < m; ++i) {
        const int64_t d = dst[i] ? accum_merge_dst(kpos[i], 0, kept) : -1;
        assert(!dst[i] || d >= 0);
        dst[i] = (int)d;
        if (d >= 0) { PCACC_BOUND(d, m); assert(rows[d] == -1); rows[d] = (int)i; }
    }
    // pass 2
    std::vector<double> n64(3 * kept), e64(3 * kept);
    std::vector<float> n32(3 * kept), e32(3 * kept);
    std::vector<int32_t> nb(kept);
    std::vector<uint8_t> fl(kept);
    for (int64_t j = 0; j < kept; ++j) {
        const int64_t i = rows[j];
        assert(i >= 0 && i < m && dst[i] == j);
        AccnResult r;
        const bool ok = accum_normal_voxel(keys.data(), acc.data(), stamps.data(), cap, m, dst.data(), i, radius, min_neighbors,
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
    assert(fwrite(&kept, 8, 1, o) == 1);
    wr(o, n64); wr(o, e64); wr(o, nb); wr(o, fl); wr(o, n32); wr(o, e32);
    fclose(o);
    fclose(f);
    return 0;
}
