// Host build of pcaccumulation_amd/csrc/accum_grid.h (tests/test_accumulate.py): the per-point arithmetic and the index arithmetic of the window
// reduction, the search and the merge -- the functions the kernels of accum.hip call -- run stage by stage on the CPU with every table index
// assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.
//   in : i64 n_adds, i64 capacity, i64 min_count, i64 use_fraction, f64 max_moving_fraction, f64 voxel_size, then per add
//        i64 n, i64 stamp, i64 has_pose, f64 pose[16], f32 points[3n], u8 moving[n]
//   out: per add and point 5 i64 (valid, key, q_x, q_y, q_z); then i64 M, dropped, growths; keys[M]; acc[5][M]; stamps[2][M] as i64;
//        then i64 V; per kept row 12 i64: coords[3], centroid bits[3], count, moving, t_first, t_last, 0, 0
#include <algorithm>

#include "accum_grid.h"
#include "accum_host.h"

// the map that grows: zeroed tables, swapped after every add
struct Tables {
    int64_t cap = 0, m = 0;
    std::vector<u64> keys;
    std::vector<int64_t> acc;
    std::vector<int32_t> stamps;
    void resize(int64_t c) { cap = c; keys.assign(c, 0); acc.assign(ACC_FIELDS * c, 0); stamps.assign(2 * c, 0); }
};

static void put(FILE *f, int64_t v) { wr1(f, v); }

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 4);
    const std::vector<double> hd = rd<double>(f, 2);
    const int64_t n_adds = h[0], min_count = h[2];
    const bool use_fraction = h[3] != 0;
    const double frac = hd[0], vs = hd[1];
    Tables cur, alt;
    cur.resize(h[1]);
    int64_t dropped_total = 0, growths = 0;
    for (int64_t a = 0; a < n_adds; ++a) {
        const std::vector<int64_t> ah = rd<int64_t>(f, 3);
        const int64_t n = ah[0];
        const int32_t stamp = (int32_t)ah[1];
        std::vector<double> pose = rd<double>(f, 16);
        if (!ah[2]) for (int k = 0; k < 16; ++k) pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
        const std::vector<float> pts = rd<float>(f, 3 * n);
        const std::vector<uint8_t> mov = rd<uint8_t>(f, n);
        if (n == 0) continue;
        // K1
        std::vector<u64> key(n);
        std::vector<int> idx(n);
        int64_t dropped = 0;
        for (int64_t i = 0; i < n; ++i) {
            u64 k;
            int64_t q[3] = {0, 0, 0};
            const bool ok = accum_point(pose.data(), &pts[3 * i], vs, &k, q);
            if (!ok) { k = ACC_INVALID_KEY; ++dropped; }
            key[i] = k;
            idx[i] = (int)i;
            put(o, ok); put(o, ok ? (int64_t)k : 0); put(o, ok ? q[0] : 0); put(o, ok ? q[1] : 0); put(o, ok ? q[2] : 0);
        }
        // K2
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return key[x] < key[y]; });
        std::vector<u64> skey(n);
        for (int64_t i = 0; i < n; ++i) skey[i] = key[idx[i]];
        // K3
        std::vector<int> head(n), vox(n + 1);
        int run_total = 0;
        for (int64_t i = 0; i < n; ++i) {
            head[i] = (skey[i] != ACC_INVALID_KEY && (i == 0 || skey[i - 1] != skey[i])) ? 1 : 0;
            vox[i] = run_total;
            run_total += head[i];
        }
        vox[n] = run_total;
        const int64_t runs = run_total;
        // K4
        std::vector<u64> wkey(n, 0);
        std::vector<int64_t> wacc(ACC_FIELDS * n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t row = accum_point_index(idx[i], n);
            if (skey[i] == ACC_INVALID_KEY || row < 0) continue;
            const int64_t run = accum_run_index(vox[i], head[i], runs);
            assert(run >= 0);
            u64 k2;
            int64_t q[3];
            const bool ok = accum_point(pose.data(), &pts[3 * row], vs, &k2, q);
            assert(ok && k2 == skey[i]);
            if (head[i]) wkey[run] = skey[i];
            const int64_t add[ACC_FIELDS] = {1, mov[row] ? 1 : 0, q[0], q[1], q[2]};
            for (int fl = 0; fl < ACC_FIELDS; ++fl) wacc[accum_field(fl, run, n)] += add[fl];
        }
        // K5
        std::vector<int> miss(n, 0), pos(n, 0), mrank(n + 1, 0);
        for (int64_t j = 0; j < runs; ++j) {
            const int64_t p = accum_lower_bound(cur.keys.data(), cur.m, wkey[j]);
            assert(p >= 0 && p <= cur.m);
            miss[j] = !(p < cur.m && cur.keys[p] == wkey[j]);
            pos[j] = (int)p;
        }
        for (int64_t j = 0; j < n; ++j) mrank[j + 1] = mrank[j] + miss[j];
        // K6: too small -> the caller doubles the output tables and calls again; nothing was written
        const int64_t total = cur.m + mrank[n];
        int64_t out_cap = cur.cap;
        while (out_cap < total) { out_cap *= 2; ++growths; }
        alt.resize(out_cap);
        // K7
        for (int64_t p = 0; p < cur.m; ++p) {
            const int64_t j = accum_lower_bound(wkey.data(), runs, cur.keys[p]);
            PCACC_BOUND(j, n + 1);
            const int64_t d = accum_merge_dst(p, mrank[j], total);
            assert(d >= 0);
            PCACC_BOUND(d, alt.cap);
            const bool hit = j < runs && wkey[j] == cur.keys[p];
            assert(alt.acc[accum_field(0, d, alt.cap)] == 0);                    // no destination is written twice
            alt.keys[d] = cur.keys[p];
            for (int fl = 0; fl < ACC_FIELDS; ++fl)
                alt.acc[accum_field(fl, d, alt.cap)] = cur.acc[accum_field(fl, p, cur.cap)] + (hit ? wacc[accum_field(fl, j, n)] : 0);
            const int32_t t0 = cur.stamps[p], t1 = cur.stamps[cur.cap + p];
            alt.stamps[d] = (hit && stamp < t0) ? stamp : t0;
            alt.stamps[alt.cap + d] = (hit && stamp > t1) ? stamp : t1;
        }
        for (int64_t j = 0; j < runs; ++j) {
            if (!miss[j]) continue;
            const int64_t d = accum_merge_dst(pos[j], mrank[j], total);
            assert(d >= 0);
            PCACC_BOUND(d, alt.cap);
            assert(alt.acc[accum_field(0, d, alt.cap)] == 0);
            alt.keys[d] = wkey[j];
            for (int fl = 0; fl < ACC_FIELDS; ++fl) alt.acc[accum_field(fl, d, alt.cap)] = wacc[accum_field(fl, j, n)];
            alt.stamps[d] = stamp;
            alt.stamps[alt.cap + d] = stamp;
        }
        alt.m = total;
        for (int64_t d = 0; d < total; ++d) {
            assert(alt.acc[accum_field(0, d, alt.cap)] > 0);                     // every destination is written
            assert(d == 0 || alt.keys[d - 1] < alt.keys[d]);                     // ascending, duplicate-free
        }
        std::swap(cur, alt);
        dropped_total += dropped;
    }
    put(o, cur.m); put(o, dropped_total); put(o, growths);
    for (int64_t i = 0; i < cur.m; ++i) put(o, (int64_t)cur.keys[i]);
    for (int fl = 0; fl < ACC_FIELDS; ++fl) for (int64_t i = 0; i < cur.m; ++i) put(o, cur.acc[accum_field(fl, i, cur.cap)]);
    for (int s = 0; s < 2; ++s) for (int64_t i = 0; i < cur.m; ++i) put(o, cur.stamps[s * cur.cap + i]);
    // extract
    std::vector<int> keep(cur.m);
    for (int64_t i = 0; i < cur.m; ++i)
        keep[i] = accum_keep(cur.acc[accum_field(0, i, cur.cap)], cur.acc[accum_field(1, i, cur.cap)], min_count, use_fraction, frac);
    const std::vector<int> kpos = scan(keep);
    const int64_t kept = kpos[cur.m];
    put(o, kept);
    int64_t written = 0;
    for (int64_t i = 0; i < cur.m; ++i) {
        if (!keep[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, kept);
        assert(d == written++);
        int32_t c[3];
        accum_unkey(cur.keys[i], c);
        const int64_t count = cur.acc[accum_field(0, i, cur.cap)];
        for (int k = 0; k < 3; ++k) put(o, c[k]);
        for (int k = 0; k < 3; ++k) {
            const float v = accum_centroid(cur.acc[accum_field(2 + k, i, cur.cap)], count);
            int32_t bits;
            memcpy(&bits, &v, 4);
            put(o, bits);
        }
        put(o, count); put(o, cur.acc[accum_field(1, i, cur.cap)]); put(o, cur.stamps[i]); put(o, cur.stamps[cur.cap + i]); put(o, 0); put(o, 0);
    }
    close_io(f, o);
    return 0;
}
