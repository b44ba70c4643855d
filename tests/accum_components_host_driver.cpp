// Host build of pcaccumulation_amd/csrc/accum_components.h and union_find.h (tests/test_accumulate_components.py): which rows take part, the edges of a
// row, the joins, the contribution of a row to its component and the rows a removal drops -- the functions the kernels of accum_components.hip call --
// run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps between them (keep flags,
// exclusive scans, dst / rows, root flags, the run over the components) are the kernels' steps.
// The edges are collected first and joined in a SCRAMBLED order (seed): the labels may not depend on it.  parent[x] <= x is asserted over the whole
// table after every join while the table has at most 4096 rows, after every 1024th join and after the last one otherwise.
// The input tables stand at their capacity with a misleading key and a record that passes every filter behind row m; every output is poison before it
// is written: every label row below kept and every component row below K is written exactly once, the rows behind them stay poison; the removal's
// destinations below `kept` are written exactly once, keys ascend, and the poison behind is untouched.
//   in : i64 m, in_capacity, out_capacity, has_pierced, has_mask, mask_rows, min_count, use_fraction, radius, min_voxels, min_points, dry_run, seed;
//        f64 max_moving_fraction; a map (see accum_host.h); u8 mask[mask_rows] (has_mask)
//   out: i64 counters[7]; i64 remove_counters[4]; i64 edges; i32 label[kept]; per component (K rows): i32 voxels; i64 points; i64 moving; i64 sum_q[K][3];
//        f32 centroid[K][3]; i32 lo[K][3]; i32 hi[K][3]; i32 t_first; i32 t_last; i32 first_row; then, unless dry_run or a status other than OK:
//        the map of rk = remove_counters[0] rows
#include <utility>

#include "accum_components.h"
#include "accum_host.h"

static void check_descending(const std::vector<int> &parent, int64_t kept)
{
    for (int64_t x = 0; x < kept; ++x) assert(parent[x] >= 0 && parent[x] <= x);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 13);
    const std::vector<double> g = rd<double>(f, 1);
    const int64_t m = h[0], cap = h[1], ocap = h[2], mask_rows = h[5], min_count = h[6], min_voxels = h[9], min_points = h[10];
    const bool has_pierced = h[3] != 0, has_mask = h[4] != 0, use_fraction = h[7] != 0, dry_run = h[11] != 0;
    const int radius = (int)h[8];
    u64 seed = (u64)h[12];
    assert(ocap >= m && ocap >= 1 && mask_rows >= 0 && radius >= 1 && radius <= ACCN_MAX_RADIUS);
    assert(min_voxels >= 0 && min_points >= 0);
    // rows past m: a key that would mislead any search that read it, a record that passes every filter
    const Map in = read_map(f, m, cap, has_pierced, Fills{0, 1000, 1000, 0x7fffffff, 0});
    const std::vector<uint8_t> mask_v = rd<uint8_t>(f, has_mask ? mask_rows : 0);
    static const uint8_t no_rows = 0;
    const uint8_t *mask = has_mask ? (mask_rows ? mask_v.data() : &no_rows) : nullptr;

    // the row table
    const RowTable filtered = row_table(in, min_count, use_fraction, g[0]);
    const std::vector<int> &dst = filtered.dst, &rows = filtered.rows;
    const int64_t kept = filtered.kept;
    const bool fits = accc_mask_fits(mask, mask_rows, kept);
    std::vector<int64_t> counters(ACCC_COUNTERS, 0), rcounters(ACCC_REMOVE_COUNTERS, 0);
    counters[ACCC_C_ROWS] = m;
    counters[ACCC_C_OUTSIDE] = m - kept;

    // edges, then the joins in a scrambled order
    std::vector<int> parent(m);
    for (int64_t j = 0; j < m; ++j) parent[j] = (int)j;
    std::vector<std::pair<int, int>> edges;
    if (!fits) {
        counters[ACCC_C_MASKED] = kept;
        counters[ACCC_C_STATUS] = ACCC_BAD_MASK;
    } else {
        for (int64_t j = 0; j < kept; ++j) {
            const int64_t i = rows[j];
            assert(i >= 0 && i < m && dst[i] == j && accc_row(dst.data(), mask, kept, i, m) == (accc_takes_part(mask, kept, j) ? j : ACCC_MASKED));
            if (!accc_takes_part(mask, kept, j)) { counters[ACCC_C_MASKED] += 1; continue; }
            counters[ACCC_C_PARTICIPATING] += 1;
            const int n = accc_edges(in.keys.data(), m, dst.data(), mask, kept, i, j, radius, [&](int64_t a, int64_t b) {
                assert(a == j && b >= 0 && b < j);
                edges.push_back(std::make_pair((int)a, (int)b));
            });
            assert(n >= 0 && n <= ((2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1) - 1) / 2);
        }
        for (size_t e = edges.size(); e > 1; --e) {                                          // Fisher-Yates on a 64-bit LCG
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(edges[e - 1], edges[(size_t)((seed >> 33) % e)]);
        }
        for (size_t e = 0; e < edges.size(); ++e) {
            const int r = uf_union_bounded(parent.data(), edges[e].first, edges[e].second, ACCC_UNION_TRIES);
            assert(r >= 0 && r <= edges[e].second);                                          // alone, the first attempt wins
            if (kept <= 4096 || e % 1024 == 1023 || e + 1 == edges.size()) check_descending(parent, kept);
        }
        for (int64_t j = 0; j < kept; ++j) {                                                 // flatten
            const int r = uf_root(parent.data(), (int)j);
            if (r != (int)j) uf_store(&parent[j], r);
        }
        check_descending(parent, kept);
    }
    assert(counters[ACCC_C_ROWS] == counters[ACCC_C_PARTICIPATING] + counters[ACCC_C_OUTSIDE] + counters[ACCC_C_MASKED]);

    // numbering
    std::vector<int> rootf(m, 0);
    for (int64_t j = 0; j < kept; ++j) rootf[j] = (fits && accc_takes_part(mask, kept, j) && parent[j] == (int)j) ? 1 : 0;
    const std::vector<int> cid = scan(rootf);
    const int64_t K = cid[m];
    counters[ACCC_C_COMPONENTS] = K;
    const int64_t tab = m + 3;                                                               // room for m rows and poison behind them
    std::vector<int32_t> label(tab, POISON_I32), voxels(tab, POISON_I32), lo(3 * tab, POISON_I32), hi(3 * tab, POISON_I32), t_first(tab, POISON_I32),
        t_last(tab, POISON_I32), first_row(tab, POISON_I32);
    std::vector<int64_t> points(tab, POISON_ACC), moving(tab, POISON_ACC), sum_q(3 * tab, POISON_ACC);
    std::vector<float> centroid(3 * tab, POISON_F32);
    std::vector<int> label_written(tab, 0), comp_written(tab, 0);
    std::vector<AcccStat> stat(K);
    for (int64_t c = 0; c < K; ++c) accc_stat_none(&stat[c]);
    for (int64_t j = 0; j < kept; ++j) {
        int32_t lab = -1;
        if (fits && accc_takes_part(mask, kept, j)) {
            const int64_t root = accn_index(parent[j], kept);
            const int64_t c = accn_index(cid[root], K);
            assert(root <= j && c >= 0);
            lab = (int32_t)c;
            if (root == j) { assert(first_row[c] == POISON_I32); first_row[c] = (int32_t)j; }
            AcccStat s;
            assert(accc_stat_row(in.keys.data(), in.acc.data(), in.stamps.data(), cap, m, rows[j], &s));
            accc_stat_merge(&stat[c], s);
        }
        PCACC_BOUND(j, tab);
        label[j] = lab;
        label_written[j] += 1;
    }
    int64_t largest = 0;
    for (int64_t c = 0; c < K; ++c) {
        const AcccStat &s = stat[c];
        assert(s.voxels >= 1 && s.points >= 1 && first_row[c] >= 0 && label[first_row[c]] == c && (c == 0 || first_row[c - 1] < first_row[c]));
        voxels[c] = (int32_t)s.voxels; points[c] = s.points; moving[c] = s.moving;
        sum_q[3 * c] = s.sq_x; sum_q[3 * c + 1] = s.sq_y; sum_q[3 * c + 2] = s.sq_z;
        centroid[3 * c] = accc_centroid(s.sq_x, s.points); centroid[3 * c + 1] = accc_centroid(s.sq_y, s.points);
        centroid[3 * c + 2] = accc_centroid(s.sq_z, s.points);
        lo[3 * c] = s.lo_x; lo[3 * c + 1] = s.lo_y; lo[3 * c + 2] = s.lo_z;
        hi[3 * c] = s.hi_x; hi[3 * c + 1] = s.hi_y; hi[3 * c + 2] = s.hi_z;
        t_first[c] = s.t_first; t_last[c] = s.t_last;
        comp_written[c] += 1;
        largest = s.voxels > largest ? s.voxels : largest;
    }
    counters[ACCC_C_LARGEST] = largest;
    for (int64_t r = 0; r < tab; ++r) {
        assert(label_written[r] == (r < kept ? 1 : 0) && comp_written[r] == (r < K ? 1 : 0));
        if (r >= kept) assert(label[r] == POISON_I32);
        if (r >= K)
            assert(voxels[r] == POISON_I32 && points[r] == POISON_ACC && moving[r] == POISON_ACC && sum_q[3 * r] == POISON_ACC && lo[3 * r + 2] == POISON_I32 &&
                   hi[3 * r] == POISON_I32 && t_first[r] == POISON_I32 && t_last[r] == POISON_I32 && first_row[r] == POISON_I32 &&
                   centroid[3 * r + 1] == POISON_F32);
    }

    // removal
    const bool ok = counters[ACCC_C_STATUS] == ACCC_OK;
    std::vector<int> flag(m);
    for (int64_t i = 0; i < m; ++i)
        flag[i] = (ok && accc_row_small(dst.data(), label.data(), voxels.data(), points.data(), kept, K, i, m, min_voxels, min_points)) ? 0 : 1;
    const std::vector<int> kpos = scan(flag);
    const int64_t rk = kpos[m];
    const bool dry = dry_run || !ok;
    Map out = poison_map(ocap, has_pierced);
    std::vector<int> written(ocap, 0);
    for (int64_t i = 0; i < m; ++i) {
        rcounters[flag[i] ? ACCC_R_KEPT : ACCC_R_SMALL] += 1;
        if (dry || !flag[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, rk);
        assert(d >= 0 && d < rk);
        assert(accr_move_row(in.keys.data(), in.acc.data(), in.stamps.data(), in.p(), cap, m, i, out.keys.data(), out.acc.data(), out.stamps.data(), out.p(),
                             ocap, rk, d));
        written[d] += 1;
    }
    for (int64_t c = 0; c < K; ++c) rcounters[(ok && accc_small(voxels[c], points[c], min_voxels, min_points)) ? ACCC_R_COMPONENTS_REMOVED : ACCC_R_COMPONENTS_KEPT] += 1;
    assert(rcounters[ACCC_R_KEPT] + rcounters[ACCC_R_SMALL] == m && rcounters[ACCC_R_KEPT] == rk);
    assert(rcounters[ACCC_R_COMPONENTS_REMOVED] + rcounters[ACCC_R_COMPONENTS_KEPT] == K);
    assert_written_once(written, dry ? 0 : rk);
    assert_poison_from(out, dry ? 0 : rk);

    wr(o, counters, ACCC_COUNTERS); wr(o, rcounters, ACCC_REMOVE_COUNTERS);
    const std::vector<int64_t> n_edges(1, (int64_t)edges.size());
    wr(o, n_edges, 1);
    wr(o, label, kept); wr(o, voxels, K); wr(o, points, K); wr(o, moving, K); wr(o, sum_q, 3 * K); wr(o, centroid, 3 * K); wr(o, lo, 3 * K); wr(o, hi, 3 * K);
    wr(o, t_first, K); wr(o, t_last, K); wr(o, first_row, K);
    if (!dry) write_map(o, out, rk);
    close_io(f, o);
    return 0;
}
