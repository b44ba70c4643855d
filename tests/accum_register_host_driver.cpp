// Host build of pcaccumulation_amd/csrc/accum_register.h (tests/test_accumulate_register.py): the whole registration -- row table, normals (C5's
// accum_normal_voxel), then every round: accr_point per scan point, accr_slot_sum per slot and term, the slots in order, accr_round -- run on the CPU
// with every table index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The tables sit at a capacity above m with poison behind
// row m.  The loop stops where the device's stops: the rounds after `done` would return at once.
//   in : i64 m, capacity, min_count, use_fraction, radius, min_neighbors, n_viewpoints, stamp_base, n, has_moving, max_iter, has_init;
//        f64 max_moving_fraction, voxel_size, max_distance; i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; f64 viewpoints[n_viewpoints][3];
//        f32 points[n][3]; u8 moving[n] (has_moving); f64 init[16] (has_init)
//   out: f64 pose[16], fitness, rmse; i32 iterations, status, correspondences; i64 V; f32 normals[V][3]; u8 flags[V];
//        i64 first[n], last[n]: the matched map row of every point (-1 = none) in the first and in the last evaluation; i64 evaluations
#include <cassert>
#include <cstdio>
#include <vector>

#include "accum_register.h"

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
    const std::vector<int64_t> h = rd<int64_t>(f, 12);
    const std::vector<double> hd = rd<double>(f, 3);
    const int64_t m = h[0], cap = h[1], min_count = h[2], n_view = h[6], stamp_base = h[7], n = h[8];
    const bool use_fraction = h[3] != 0, has_moving = h[9] != 0, has_init = h[11] != 0;
    const int radius = (int)h[4], min_neighbors = (int)h[5], max_iter = (int)h[10];
    const double frac = hd[0], voxel_size = hd[1], max_distance = hd[2];
    assert(m >= 0 && cap >= m && cap >= 1 && radius >= 1 && radius <= ACCN_MAX_RADIUS && min_neighbors >= ACCN_MIN_NEIGHBORS && n_view >= 0);
    assert(n >= 0 && max_iter >= 0 && voxel_size > 0.0 && max_distance > 0.0 && max_distance <= voxel_size);
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
    const std::vector<float> points = rd<float>(f, 3 * n);
    const std::vector<uint8_t> moving = rd<uint8_t>(f, has_moving ? n : 0);
    const std::vector<double> init = rd<double>(f, has_init ? 16 : 0);
    // the row table (pass 1 of C5) and the normals of the kept rows
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
    std::vector<float> n32(3 * kept);
    std::vector<uint8_t> fl(kept);
    int64_t candidates = 0;
    for (int64_t j = 0; j < kept; ++j) {
        AccnResult r;
        const bool ok = accum_normal_voxel(keys.data(), acc.data(), stamps.data(), cap, m, dst.data(), rows[j], radius, min_neighbors,
                                           n_view > 0 ? view.data() : nullptr, n_view, stamp_base, &r);
        assert(ok);
        for (int a = 0; a < 3; ++a) n32[3 * j + a] = (float)r.normal[a];
        fl[j] = (uint8_t)r.flags;
        if (!(r.flags & 3)) ++candidates;
    }
    int64_t eligible = n;
    if (has_moving) {
        eligible = 0;
        for (int64_t i = 0; i < n; ++i) eligible += moving[i] ? 0 : 1;
    }
    // the rounds
    AccrState st;
    accr_init(&st, has_init ? init.data() : nullptr, eligible, candidates);
    double pose[16], fitness = -1.0, rmse = -1.0;
    int32_t iterations = -1, status = -1, correspondences = -1;
    const AccrOut out = {pose, &fitness, &rmse, &iterations, &status, &correspondences};
    const int64_t slots = (m > 0 && kept > 0) ? (n + ACCR_SLOT - 1) / ACCR_SLOT : 0;
    const double max_d2 = max_distance * max_distance;
    std::vector<int64_t> first(n, -1), last(n, -1);
    std::vector<double> partial(slots * ACCR_TERMS), terms((size_t)ACCR_SLOT * ACCR_TERMS);
    int64_t evaluations = 0;
    for (int round = 0; round <= max_iter && !st.done; ++round) {
        for (int64_t s = 0; s < slots; ++s) {
            for (int l = 0; l < ACCR_SLOT; ++l) {
                double *t = &terms[(size_t)l * ACCR_TERMS];
                const int64_t i = s * ACCR_SLOT + l;
                if (i < n) {
                    int64_t row;
                    accr_point(keys.data(), acc.data(), cap, m, dst.data(), n32.data(), fl.data(), kept, st.T, points.data(),
                               has_moving ? moving.data() : nullptr, n, i, voxel_size, max_d2, t, &row);
                    assert(row >= -1 && row < m);
                    if (round == 0) first[i] = row;
                    last[i] = row;
                } else {
                    for (int k = 0; k < ACCR_TERMS; ++k) t[k] = 0.0;
                }
            }
            for (int k = 0; k < ACCR_TERMS; ++k) {
                double v[ACCR_SLOT];
                for (int l = 0; l < ACCR_SLOT; ++l) v[l] = terms[(size_t)l * ACCR_TERMS + k];
                partial[s * ACCR_TERMS + k] = accr_slot_sum(v);
            }
        }
        double sums[ACCR_TERMS];
        for (int k = 0; k < ACCR_TERMS; ++k) {
            double v = 0.0;
            for (int64_t s = 0; s < slots; ++s) v = v + partial[s * ACCR_TERMS + k];
            sums[k] = v;
        }
        ++evaluations;
        accr_round(&st, sums, round, max_iter, &out);
    }
    assert(st.done && iterations >= 0 && iterations <= max_iter && correspondences >= 0 && correspondences <= n);
    wr(o, std::vector<double>(pose, pose + 16));
    assert(fwrite(&fitness, 8, 1, o) == 1 && fwrite(&rmse, 8, 1, o) == 1);
    assert(fwrite(&iterations, 4, 1, o) == 1 && fwrite(&status, 4, 1, o) == 1 && fwrite(&correspondences, 4, 1, o) == 1);
    assert(fwrite(&kept, 8, 1, o) == 1);
    wr(o, n32); wr(o, fl); wr(o, first); wr(o, last);
    assert(fwrite(&evaluations, 8, 1, o) == 1);
    fclose(o);
    fclose(f);
    return 0;
}
