// Host build of pcaccumulation_amd/csrc/accum_columns.h (tests/test_accumulate_columns.py): the whole route of accum_columns.hip -- row table, head flags,
// scan, then accc_column per head, accc_ground per column, the row outputs and accc_band per head, and accc_pixel per pixel of every window, the
// functions the kernels call -- run on the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The map's
// tables stand at a capacity above m with poison behind row m that no result may depend on (a key that would mislead any search that read it, a record
// that passes every filter); every output is poison before the loops, and every element of every output is asserted written exactly once.
//   in : i64 m, capacity, min_count, use_fraction, radius, thickness, band_lo, band_hi, n_windows; f64 max_moving_fraction; a map with stamps (see
//        accum_host.h); i64 windows[n_windows][4] = x0, y0, W, H
//   out: i64 counters[5]; i64 V (rows the filter keeps); i64 C; the column tables (C rows each): i64 key; i32 xy[C][2], first_row, voxels; i64 points,
//        moving; i32 z_low, z_high, t_first, t_last, ground_z, ground_row, ground_column, band_voxels, band_top; the row tables (V rows each):
//        i32 column, height; u8 is_ground; f64 height_m; per window: i32 column[H][W]; f32 elevation, ground; i32 band_top, voxels
#include "accum_columns.h"
#include "accum_host.h"

template <class T> static void put(std::vector<T> &v, std::vector<int> &written, int64_t i, const T &x)
{
    PCACC_BOUND(i, (int64_t)v.size());
    assert(is_poison(v[i]));
    v[i] = x;
    written[i] += 1;
}

static void all_once(const std::vector<int> &written)
{
    for (size_t d = 0; d < written.size(); ++d) assert(written[d] == 1);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const std::vector<double> g = rd<double>(f, 1);
    const int64_t m = h[0], cap = h[1], min_count = h[2], n_windows = h[8];
    const bool use_fraction = h[3] != 0;
    const int R = (int)h[4], thickness = (int)h[5], band_lo = (int)h[6], band_hi = (int)h[7];
    assert(R >= 0 && R <= ACCC_MAX_RADIUS && thickness >= 0 && thickness <= ACCC_MAX_HEIGHT && band_lo >= 0 && band_lo <= band_hi && band_hi <= ACCC_MAX_HEIGHT);
    const Map map = read_map(f, m, cap, false, Fills{0, 1000, 0, -0x7fffffff, 77});
    const std::vector<int64_t> windows = rd<int64_t>(f, 4 * n_windows);
    const RowTable tab = row_table(map, min_count, use_fraction, g[0]);                         // pass 1 of C5
    const int64_t kept = tab.kept;

    AcccMap M;
    M.keys = map.keys.data(); M.acc = map.acc.data(); M.stamps = map.stamps.data(); M.rows = tab.rows.data();
    M.capacity = cap; M.m = m; M.kept = kept;

    std::vector<int> head(m, 0);                                                                // 0 behind the kept rows, as the kernel writes it
    for (int64_t j = 0; j < kept; ++j) head[j] = accc_is_head(M, j) ? 1 : 0;
    const std::vector<int> cpos = scan(head);
    const int64_t C = cpos[m];
    assert(C <= kept && (C > 0) == (kept > 0));

    std::vector<int64_t> key = poisoned<int64_t>(C), points = poisoned<int64_t>(C), moving = poisoned<int64_t>(C);
    std::vector<int32_t> xy = poisoned<int32_t>(2 * C), first_row = poisoned<int32_t>(C), voxels = poisoned<int32_t>(C), z_low = poisoned<int32_t>(C),
                         z_high = poisoned<int32_t>(C), t_first = poisoned<int32_t>(C), t_last = poisoned<int32_t>(C), ground_z = poisoned<int32_t>(C),
                         ground_row = poisoned<int32_t>(C), ground_column = poisoned<int32_t>(C), band_voxels = poisoned<int32_t>(C),
                         band_top = poisoned<int32_t>(C);
    std::vector<int> w_col(C, 0), w_xy(2 * C, 0), w_ground(C, 0), w_band(C, 0), w_row(kept, 0);
    std::vector<int64_t> counters(ACCC_COUNTERS, 0);

    // the column kernel: the lane of a head walks its run
    int64_t covered = 0;
    for (int64_t j = 0; j < kept; ++j) {
        if (!head[j]) continue;
        const int64_t c = accum_run_index(cpos[j], 1, C);
        assert(c >= 0);
        AcccColumn col;
        assert(accc_column(M, j, &col));
        assert(col.first_row == j && col.voxels >= 1 && j == covered && col.z_low <= col.z_high && col.t_first <= col.t_last);
        assert(col.z_high - col.z_low >= col.voxels - 1 && col.points >= col.voxels && col.moving >= 0 && col.moving <= col.points);
        covered += col.voxels;                                                                  // the runs tile the kept rows
        assert(is_poison(key[c]));
        key[c] = (int64_t)col.key; points[c] = col.points; moving[c] = col.moving;
        put(xy, w_xy, 2 * c, col.xy[0]); put(xy, w_xy, 2 * c + 1, col.xy[1]);
        first_row[c] = col.first_row; voxels[c] = col.voxels; z_low[c] = col.z_low; z_high[c] = col.z_high; t_first[c] = col.t_first; t_last[c] = col.t_last;
        w_col[c] += 1;
    }
    assert(covered == kept);
    all_once(w_col); all_once(w_xy);
    for (int64_t c = 1; c < C; ++c) assert((u64)key[c - 1] < (u64)key[c]);                      // the compact list ascends: what the searches rely on

    // the ground kernel: one lane per column
    for (int64_t c = 0; c < C; ++c) {
        const int64_t s = accc_ground((const u64 *)key.data(), z_low.data(), C, c, R);
        assert(s >= 0 && s < C && z_low[s] <= z_low[c]);
        assert(xy[2 * s] - xy[2 * c] <= R && xy[2 * c] - xy[2 * s] <= R && xy[2 * s + 1] - xy[2 * c + 1] <= R && xy[2 * c + 1] - xy[2 * s + 1] <= R);
        assert(is_poison(ground_z[c]) && is_poison(ground_row[c]) && is_poison(ground_column[c]));
        ground_z[c] = z_low[s]; ground_row[c] = first_row[s]; ground_column[c] = (int32_t)s;
        w_ground[c] += 1;
        counters[ACCC_C_COLUMNS] += 1;
        counters[ACCC_C_BORROWED] += s != c;
    }
    all_once(w_ground);

    // the row / band kernel: one lane per kept row, the lane of a head owns the band of its column
    std::vector<int32_t> r_column = poisoned<int32_t>(kept), r_height = poisoned<int32_t>(kept);
    std::vector<uint8_t> r_ground = poisoned<uint8_t>(kept);
    std::vector<double> r_height_m = poisoned<double>(kept);
    for (int64_t j = 0; j < kept; ++j) {
        const int64_t c = accum_run_index(cpos[j], head[j], C);
        int32_t z;
        assert(c >= 0 && accc_row_z(M, j, &z));
        PCACC_BOUND(c, C);
        assert(j >= first_row[c] && j < first_row[c] + voxels[c]);
        const int32_t height = z - ground_z[c];
        assert(height >= 0 && height <= ACCC_MAX_HEIGHT);
        assert(is_poison(r_column[j]) && is_poison(r_height[j]) && is_poison(r_ground[j]) && is_poison(r_height_m[j]));
        r_column[j] = (int32_t)c; r_height[j] = height; r_ground[j] = height <= thickness ? 1 : 0;
        r_height_m[j] = accc_height_m(M, j, ground_row[c]);
        assert(r_height_m[j] == r_height_m[j]);                                                 // both rows exist: no NaN
        w_row[j] += 1;
        counters[ACCC_C_ROWS] += 1;
        counters[ACCC_C_GROUND] += height <= thickness;
        if (head[j]) {
            int32_t top;
            const int32_t n = accc_band(M, j, voxels[c], ground_z[c], band_lo, band_hi, &top);
            assert(n >= 0 && n <= voxels[c] && (n == 0) == (top == -1) && (n == 0 || (top >= band_lo && top <= band_hi)));
            assert(is_poison(band_voxels[c]) && is_poison(band_top[c]));
            band_voxels[c] = n; band_top[c] = top;
            w_band[c] += 1;
            counters[ACCC_C_BAND] += n;
        }
    }
    all_once(w_row); all_once(w_band);

    wr(o, counters);
    wr1(o, kept);
    wr1(o, C);
    wr(o, key); wr(o, xy); wr(o, first_row); wr(o, voxels); wr(o, points); wr(o, moving); wr(o, z_low); wr(o, z_high); wr(o, t_first); wr(o, t_last);
    wr(o, ground_z); wr(o, ground_row); wr(o, ground_column); wr(o, band_voxels); wr(o, band_top);
    wr(o, r_column); wr(o, r_height); wr(o, r_ground); wr(o, r_height_m);

    // the pixel kernel: one lane per pixel
    const AcccColumns T = {(const u64 *)key.data(), first_row.data(), voxels.data(), ground_row.data(), band_top.data(), C};
    AcccMap P = M;
    P.stamps = nullptr;                                                                          // a pixel reads no stamp
    for (int64_t w = 0; w < n_windows; ++w) {
        const int64_t x0 = windows[4 * w], y0 = windows[4 * w + 1], W = windows[4 * w + 2], H = windows[4 * w + 3];
        assert(W >= 1 && H >= 1 && W * H <= ACCC_MAX_PIXELS && x0 >= -ACCC_MAX_ORIGIN && x0 <= ACCC_MAX_ORIGIN && y0 >= -ACCC_MAX_ORIGIN && y0 <= ACCC_MAX_ORIGIN);
        const int64_t n = W * H;
        std::vector<int32_t> i_column = poisoned<int32_t>(n), i_top = poisoned<int32_t>(n), i_voxels = poisoned<int32_t>(n);
        std::vector<float> i_elevation = poisoned<float>(n), i_ground = poisoned<float>(n);
        std::vector<int> w_px(n, 0);
        for (int64_t p = 0; p < n; ++p) {
            const int64_t r = p / W, c = p - r * W;
            AcccPixel px;
            accc_pixel(P, T, x0 + c, y0 + r, &px);
            assert(px.column >= -1 && px.column < C);
            if (px.column >= 0) assert(xy[2 * px.column] == x0 + c && xy[2 * px.column + 1] == y0 + r && px.elevation == px.elevation && px.ground == px.ground);
            else assert(px.elevation != px.elevation && px.ground != px.ground && px.band_top == -1 && px.voxels == 0);
            assert(is_poison(i_column[p]) && is_poison(i_elevation[p]) && is_poison(i_ground[p]) && is_poison(i_top[p]) && is_poison(i_voxels[p]));
            i_column[p] = px.column; i_elevation[p] = px.elevation; i_ground[p] = px.ground; i_top[p] = px.band_top; i_voxels[p] = px.voxels;
            w_px[p] += 1;
        }
        all_once(w_px);
        wr(o, i_column); wr(o, i_elevation); wr(o, i_ground); wr(o, i_top); wr(o, i_voxels);
    }
    close_io(f, o);
    return 0;
}
