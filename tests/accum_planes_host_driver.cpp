// Host build of pcaccumulation_amd/csrc/accum_planes.h with accum_components.h and union_find.h (tests/test_accumulate_planes.py): which rows take
// part, the gated edges of a row, the joins, the integer moments of a segment, its plane and every row's distance to it -- the functions the kernels
// of accum_planes.hip call -- run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps
// between them (keep flags, exclusive scans, dst / rows, root flags, the runs over the segments) are the kernels' steps.
// Every candidate pair is tested from both ends (the rule is symmetric bit for bit).  The gated edges are collected first and joined in a SCRAMBLED
// order (seed), each presented from its larger or its smaller end as the seed decides (flip = 1 exchanges the two): the labels may depend on
// neither.  parent[x] <= x is asserted over the whole table after every join while the table has at most 4096 rows, after every 1024th join and
// after the last one otherwise.  The input tables stand at their capacity with a misleading key and a record that passes every filter behind row m;
// every output is poison before it is written: every row table below kept and every segment table below K is written exactly once, the rows behind
// stay poison.
//   in : i64 m, capacity, has_mask, mask_rows, n_rows, min_count, use_fraction, radius, seed, flip; f64 max_moving_fraction, cos_angle, max_offset,
//        max_variation; a map (see accum_host.h); u8 mask[mask_rows] (has_mask); f32 normals[n_rows][3]; f32 eigenvalues[n_rows][3]; u8 flags[n_rows]
//   out: i64 counters[9]; i64 candidate pairs; i64 edges; i32 label[kept]; f64 distance[kept]; per segment (K rows): i32 voxels; i64 points;
//        i32 lo[K][3]; i32 hi[K][3]; i32 first_row; i32 t_first; i32 t_last; i32 anchor[K][3]; i64 spread; i32 shift; i64 s1[K][3]; i64 s2[K][6];
//        f64 normal[K][3]; f64 eigenvalues[K][3]; f64 centroid[K][3]; f64 offset; f64 mse; u8 flags
#include <utility>

#include "accum_planes.h"
#include "accum_host.h"

static void check_descending(const std::vector<int> &parent, int64_t kept)
{
    for (int64_t x = 0; x < kept; ++x) assert(parent[x] >= 0 && parent[x] <= x);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 10);
    const std::vector<double> g = rd<double>(f, 4);
    const int64_t m = h[0], cap = h[1], mask_rows = h[3], n_rows = h[4], min_count = h[5];
    const bool has_mask = h[2] != 0, use_fraction = h[6] != 0, flip = h[9] != 0;
    const int radius = (int)h[7];
    u64 seed = (u64)h[8];
    const double cos_angle = g[1], max_offset = g[2], max_variation = g[3];
    assert(mask_rows >= 0 && n_rows >= 0 && radius >= 1 && radius <= ACCN_MAX_RADIUS);
    assert(cos_angle >= 0.0 && cos_angle <= 1.0 && max_offset >= 0.0 && max_variation >= 0.0 && max_variation <= 1.0);
    // rows past m: a key that would mislead any search that read it, a record that passes every filter
    const Map in = read_map(f, m, cap, false, Fills{0, 1000, 1000, 0x7fffffff, 0});
    const std::vector<uint8_t> mask_v = rd<uint8_t>(f, has_mask ? mask_rows : 0);
    const std::vector<float> normals = rd<float>(f, 3 * n_rows), eigenvalues = rd<float>(f, 3 * n_rows);
    const std::vector<uint8_t> flags = rd<uint8_t>(f, n_rows);
    static const uint8_t no_rows = 0;
    const uint8_t *mask = has_mask ? (mask_rows ? mask_v.data() : &no_rows) : nullptr;

    // the row table and the rows that take part
    const RowTable filtered = row_table(in, min_count, use_fraction, g[0]);
    const std::vector<int> &dst = filtered.dst, &rows = filtered.rows;
    const int64_t kept = filtered.kept;
    const bool fits = acpl_rows_fit(mask, mask_rows, n_rows, kept);
    std::vector<int64_t> counters(ACPL_COUNTERS, 0);
    counters[ACPL_C_ROWS] = m;
    counters[ACPL_C_OUTSIDE] = m - kept;
    std::vector<uint8_t> part(m + 1, 0);                                                     // never empty: accc_takes_part reads a NULL mask as "all"
    if (!fits) {
        counters[ACPL_C_MASKED] = kept;
        counters[ACPL_C_STATUS] = ACPL_BAD_ROWS;
    } else {
        for (int64_t j = 0; j < kept; ++j) {
            const int cls = acpl_class(mask, flags.data(), eigenvalues.data(), kept, j, max_variation);
            assert(cls <= ACPL_TAKES_PART && cls >= ACPL_NOT_FLAT && cls != ACPL_OUTSIDE);
            part[j] = cls == ACPL_TAKES_PART ? 1 : 0;
            counters[cls == ACPL_TAKES_PART ? ACPL_C_PARTICIPATING : cls == ACPL_MASKED ? ACPL_C_MASKED : cls == ACPL_INVALID ? ACPL_C_INVALID : ACPL_C_NOT_FLAT] += 1;
        }
    }
    assert(counters[ACPL_C_ROWS] == counters[ACPL_C_PARTICIPATING] + counters[ACPL_C_OUTSIDE] + counters[ACPL_C_MASKED] + counters[ACPL_C_INVALID] +
                                        counters[ACPL_C_NOT_FLAT]);

    // candidate pairs, the rule from both ends, then the joins in a scrambled order
    std::vector<int> parent(m);
    for (int64_t j = 0; j < m; ++j) parent[j] = (int)j;
    std::vector<std::pair<int, int>> edges;
    int64_t candidates = 0;
    for (int64_t j = 0; fits && j < kept; ++j) {
        const int64_t i = rows[j];
        assert(i >= 0 && i < m && dst[i] == j);
        AcplRow mine;
        if (!accc_takes_part(part.data(), kept, j)) continue;
        assert(acpl_row(in.acc.data(), cap, m, i, normals.data(), kept, j, &mine));
        const int n = accc_edges(in.keys.data(), m, dst.data(), part.data(), kept, i, j, radius, [&](int64_t a, int64_t b) {
            assert(a == j && b >= 0 && b < j && part[b] != 0);
            const int64_t p = accn_index(rows[b], m);
            AcplRow other;
            assert(p >= 0 && p < i && dst[p] == b && acpl_row(in.acc.data(), cap, m, p, normals.data(), kept, b, &other));
            const bool joined = acpl_joined(mine, other, cos_angle, max_offset);
            assert(joined == acpl_joined(other, mine, cos_angle, max_offset));               // symmetric: either end decides alike
            if (joined) edges.push_back(std::make_pair((int)a, (int)b));
        });
        assert(n >= 0 && n <= ((2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1) - 1) / 2);
        candidates += n;
    }
    for (size_t e = edges.size(); e > 1; --e) {                                              // Fisher-Yates on a 64-bit LCG
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(edges[e - 1], edges[(size_t)((seed >> 33) % e)]);
    }
    for (size_t e = 0; e < edges.size(); ++e) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const bool swap_ends = (((seed >> 40) & 1) != 0) != flip;
        const int a = swap_ends ? edges[e].second : edges[e].first, b = swap_ends ? edges[e].first : edges[e].second;
        const int r = uf_union_bounded(parent.data(), a, b, ACCC_UNION_TRIES);
        assert(r >= 0 && r <= edges[e].second);                                              // alone, the first attempt wins
        if (kept <= 4096 || e % 1024 == 1023 || e + 1 == edges.size()) check_descending(parent, kept);
    }
    for (int64_t j = 0; j < kept; ++j) {                                                     // flatten
        const int r = uf_root(parent.data(), (int)j);
        if (r != (int)j) uf_store(&parent[j], r);
    }
    check_descending(parent, kept);

    // numbering
    std::vector<int> rootf(m, 0);
    for (int64_t j = 0; j < kept; ++j) rootf[j] = (accc_takes_part(part.data(), kept, j) && parent[j] == (int)j) ? 1 : 0;
    const std::vector<int> cid = scan(rootf);
    const int64_t K = cid[m];
    assert(K <= kept);
    counters[ACPL_C_SEGMENTS] = K;
    const int64_t tab = m + 3;                                                               // room for m rows and poison behind them
    std::vector<int32_t> label(tab, POISON_I32), voxels(tab, POISON_I32), lo(3 * tab, POISON_I32), hi(3 * tab, POISON_I32), t_first(tab, POISON_I32),
        t_last(tab, POISON_I32), first_row(tab, POISON_I32), anchor(3 * tab, POISON_I32), shift(tab, POISON_I32);
    std::vector<int64_t> points(tab, POISON_ACC), spread(tab, POISON_ACC), s1(3 * tab, POISON_ACC), s2(6 * tab, POISON_ACC);
    std::vector<double> distance(tab, POISON_F64), normal(3 * tab, POISON_F64), eig(3 * tab, POISON_F64), centroid(3 * tab, POISON_F64),
        offset(tab, POISON_F64), mse(tab, POISON_F64);
    std::vector<uint8_t> seg_flags(tab, POISON_U8);
    std::vector<int> label_written(tab, 0), distance_written(tab, 0), seg_written(tab, 0), fit_written(tab, 0);

    // labels, first rows and anchors
    for (int64_t j = 0; j < kept; ++j) {
        int32_t lab = -1;
        if (accc_takes_part(part.data(), kept, j)) {
            const int64_t root = accn_index(parent[j], kept);
            const int64_t c = accn_index(cid[root], K);
            assert(root <= j && c >= 0);
            lab = (int32_t)c;
            if (root == j) {
                int64_t ux, uy, uz;
                assert(first_row[c] == POISON_I32 && acpl_int_centroid(in.acc.data(), cap, m, rows[j], &ux, &uy, &uz));
                assert(ux > -((int64_t)1 << 31) && ux < ((int64_t)1 << 31) && uy > -((int64_t)1 << 31) && uy < ((int64_t)1 << 31) &&
                       uz > -((int64_t)1 << 31) && uz < ((int64_t)1 << 31));
                first_row[c] = (int32_t)j;
                anchor[3 * c] = (int32_t)ux; anchor[3 * c + 1] = (int32_t)uy; anchor[3 * c + 2] = (int32_t)uz;
            }
        }
        PCACC_BOUND(j, tab);
        label[j] = lab;
        label_written[j] += 1;
    }

    // pass 1
    std::vector<AcccStat> stat(K);
    std::vector<uint64_t> dmax(K, 0);
    for (int64_t c = 0; c < K; ++c) accc_stat_none(&stat[c]);
    for (int64_t j = 0; j < kept; ++j) {
        if (label[j] < 0) continue;
        const int64_t c = accn_index(label[j], K);
        AcccStat s;
        int64_t ux, uy, uz;
        assert(accc_stat_row(in.keys.data(), in.acc.data(), in.stamps.data(), cap, m, rows[j], &s));
        assert(acpl_int_centroid(in.acc.data(), cap, m, rows[j], &ux, &uy, &uz));
        accc_stat_merge(&stat[c], s);
        const uint64_t d = acpl_spread(ux, uy, uz, anchor[3 * c], anchor[3 * c + 1], anchor[3 * c + 2]);
        assert(d < ((uint64_t)1 << 32));
        dmax[c] = d > dmax[c] ? d : dmax[c];
    }
    int64_t largest = 0;
    for (int64_t c = 0; c < K; ++c) {
        const AcccStat &s = stat[c];
        assert(s.voxels >= 1 && s.points >= 1 && first_row[c] >= 0 && label[first_row[c]] == c && (c == 0 || first_row[c - 1] < first_row[c]));
        voxels[c] = (int32_t)s.voxels; points[c] = s.points;
        lo[3 * c] = s.lo_x; lo[3 * c + 1] = s.lo_y; lo[3 * c + 2] = s.lo_z;
        hi[3 * c] = s.hi_x; hi[3 * c + 1] = s.hi_y; hi[3 * c + 2] = s.hi_z;
        t_first[c] = s.t_first; t_last[c] = s.t_last;
        spread[c] = (int64_t)dmax[c];
        shift[c] = acpl_shift(dmax[c], s.voxels);
        const uint64_t t = (dmax[c] >> shift[c]) + 1;                                        // the promise of the shift: no sum of pass 2 leaves int64
        assert(shift[c] >= 0 && shift[c] <= ACPL_MAX_SHIFT && t <= ((uint64_t)1 << 31) && t * t <= (((uint64_t)1 << 62) / (uint64_t)s.voxels));
        assert(shift[c] == 0 || ((dmax[c] >> (shift[c] - 1)) + 1 > ((uint64_t)1 << 31)) ||
               ((dmax[c] >> (shift[c] - 1)) + 1) * ((dmax[c] >> (shift[c] - 1)) + 1) > (((uint64_t)1 << 62) / (uint64_t)s.voxels));
        seg_written[c] += 1;
        largest = s.voxels > largest ? s.voxels : largest;
    }
    counters[ACPL_C_LARGEST] = largest;

    // pass 2 and the fit
    std::vector<AcplMoments> mom(K);
    for (int64_t c = 0; c < K; ++c) acpl_moments_none(&mom[c]);
    for (int64_t j = 0; j < kept; ++j) {
        if (label[j] < 0) continue;
        const int64_t c = accn_index(label[j], K);
        int64_t ux, uy, uz;
        AcplMoments q;
        assert(acpl_int_centroid(in.acc.data(), cap, m, rows[j], &ux, &uy, &uz));
        acpl_moments_row(ux, uy, uz, anchor[3 * c], anchor[3 * c + 1], anchor[3 * c + 2], shift[c], &q);
        const int64_t t = (int64_t)(dmax[c] >> shift[c]) + 1;
        assert(q.x >= -t && q.x <= t && q.y >= -t && q.y <= t && q.z >= -t && q.z <= t);
        acpl_moments_merge(&mom[c], q);
    }
    for (int64_t c = 0; c < K; ++c) {
        const AcplMoments &q = mom[c];
        s1[3 * c] = q.x; s1[3 * c + 1] = q.y; s1[3 * c + 2] = q.z;
        s2[6 * c] = q.xx; s2[6 * c + 1] = q.xy; s2[6 * c + 2] = q.xz; s2[6 * c + 3] = q.yy; s2[6 * c + 4] = q.yz; s2[6 * c + 5] = q.zz;
        AcplFit fit;
        acpl_fit(&anchor[3 * c], shift[c], voxels[c], &s1[3 * c], &s2[6 * c], &fit);
        for (int k = 0; k < 3; ++k) { normal[3 * c + k] = fit.normal[k]; eig[3 * c + k] = fit.eigenvalues[k]; centroid[3 * c + k] = fit.centroid[k]; }
        offset[c] = fit.offset; mse[c] = fit.mse; seg_flags[c] = (uint8_t)fit.flags;
        fit_written[c] += 1;
    }
    for (int64_t j = 0; j < kept; ++j) {
        double d = 0.0;
        if (label[j] >= 0 && (seg_flags[accn_index(label[j], K)] & ACPL_PLANE_DEGENERATE) == 0) {
            const int64_t c = label[j];
            d = acpl_distance(in.acc.data(), cap, m, rows[j], normal[3 * c], normal[3 * c + 1], normal[3 * c + 2], offset[c]);
        }
        distance[j] = d;
        distance_written[j] += 1;
    }
    for (int64_t r = 0; r < tab; ++r) {
        assert(label_written[r] == (r < kept ? 1 : 0) && distance_written[r] == (r < kept ? 1 : 0));
        assert(seg_written[r] == (r < K ? 1 : 0) && fit_written[r] == (r < K ? 1 : 0));
        if (r >= kept) assert(label[r] == POISON_I32 && distance[r] == POISON_F64);
        if (r >= K)
            assert(voxels[r] == POISON_I32 && points[r] == POISON_ACC && lo[3 * r + 2] == POISON_I32 && hi[3 * r] == POISON_I32 && t_first[r] == POISON_I32 &&
                   t_last[r] == POISON_I32 && first_row[r] == POISON_I32 && anchor[3 * r + 1] == POISON_I32 && spread[r] == POISON_ACC &&
                   shift[r] == POISON_I32 && s1[3 * r + 2] == POISON_ACC && s2[6 * r + 5] == POISON_ACC && normal[3 * r] == POISON_F64 &&
                   eig[3 * r + 1] == POISON_F64 && centroid[3 * r + 2] == POISON_F64 && offset[r] == POISON_F64 && mse[r] == POISON_F64 &&
                   seg_flags[r] == POISON_U8);
    }

    wr(o, counters, ACPL_COUNTERS);
    const std::vector<int64_t> n_edges = {candidates, (int64_t)edges.size()};
    wr(o, n_edges, 2);
    wr(o, label, kept); wr(o, distance, kept);
    wr(o, voxels, K); wr(o, points, K); wr(o, lo, 3 * K); wr(o, hi, 3 * K); wr(o, first_row, K); wr(o, t_first, K); wr(o, t_last, K); wr(o, anchor, 3 * K);
    wr(o, spread, K); wr(o, shift, K); wr(o, s1, 3 * K); wr(o, s2, 6 * K); wr(o, normal, 3 * K); wr(o, eig, 3 * K); wr(o, centroid, 3 * K);
    wr(o, offset, K); wr(o, mse, K); wr(o, seg_flags, K);
    close_io(f, o);
    return 0;
}
