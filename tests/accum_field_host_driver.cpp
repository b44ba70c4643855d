// Host build of pcaccumulation_amd/csrc/accum_field.h (tests/test_accumulate_field.py): the whole route of accum_field.hip -- row table, the site grid, the
// windowed min-plus passes along z (not when planar), y and x, the cut, and the lookup of rows in the two grids, the functions the kernels call -- run on
// the CPU with every index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The map's tables stand at a capacity above m with poison
// behind row m that no result may depend on; every output of every pass is poison before the loop, with poison behind it that must still stand after it,
// and every element is asserted written exactly once.  Each pass runs twice: cell by cell straight from the grid (accf_pass_cell: the direct kernel), and
// along the contiguous axis with the chunks visited in a scrambled order, each staged into a poisoned buffer first as the line kernel stages its
// in LDS (accf_chunk_span, accf_line_min on the staged part); the two must agree in every word.
//   in : i64 m, capacity, min_count, use_fraction, R, planar, x0, y0, z0, nx, ny, nz, n_points, n_coords; f64 max_moving_fraction, voxel_size, pose[16];
//        a map without stamps (see accum_host.h); f32 points[n_points][3]; i32 coords[n_coords][3]
//   out: i64 counters[4]; i32 dist2[cells], nearest[cells]; then for the points and again for the coords: i64 counters[4]; u8 status[n]; i32 dist2[n], row[n]
#include "accum_field.h"
#include "accum_host.h"

#define BEHIND 16                                                                               // poisoned words behind every output

static void all_once(const std::vector<int> &written)
{
    for (size_t d = 0; d < written.size(); ++d) assert(written[d] == 1);
}

template <class T> static void behind_untouched(const std::vector<T> &v, int64_t n)
{
    assert((int64_t)v.size() == n + BEHIND);
    for (int64_t d = n; d < n + BEHIND; ++d) assert(is_poison(v[d]));
}

// A permutation of [0, n) that is not the identity for n > 2: the order in which the chunks or tiles are visited.
static std::vector<int64_t> scrambled(int64_t n)
{
    std::vector<int64_t> order(n);
    u64 s = 0x9e3779b97f4a7c15ull;
    for (int64_t i = 0; i < n; ++i) order[i] = n - 1 - i;
    for (int64_t i = n - 1; i > 0; --i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(order[i], order[(int64_t)((s >> 33) % (u64)(i + 1))]);
    }
    return order;
}

// One pass, both ways.  -> the output grid (cells words, the poison behind it checked and dropped).
static std::vector<u64> pass(const std::vector<u64> &in, int64_t cells, int64_t stride, int64_t len, int R)
{
    assert(cells % (stride * len) == 0);
    std::vector<u64> direct = poisoned<u64>(cells + BEHIND), staged = poisoned<u64>(cells + BEHIND);
    std::vector<int> w_direct(cells, 0), w_staged(cells, 0);
    for (int64_t e = 0; e < cells; ++e) {
        assert(is_poison(direct[e]));
        direct[e] = accf_pass_cell(in.data(), cells, stride, len, e, R);
        w_direct[e] += 1;
    }
    all_once(w_direct);
    behind_untouched(direct, cells);
    // The same windows walked DOWNWARDS.  Rows ascend with the coordinates, so an upward walk meets the lowest row of a tie first and would be right
    // even under "the first met wins"; walked downwards the lowest row is the LAST met, and the packed minimum must still report it.
    for (int64_t e = 0; e < cells; ++e) {
        const int64_t i = (e / stride) % len, base = e - i * stride;
        const int64_t lo = i - R < 0 ? 0 : i - R, hi = i + R > len - 1 ? len - 1 : i + R;
        u64 best = ACCF_NONE;
        for (int64_t j = hi; j >= lo; --j) {
            PCACC_BOUND(base + j * stride, cells);
            const u64 v = accf_candidate(in[base + j * stride], i - j);
            best = v < best ? v : best;
        }
        assert(best == direct[e]);
    }
    if (stride == 1) {                                                                           // the line kernel
        const int64_t chunks = (cells + ACCF_CHUNK - 1) / ACCF_CHUNK;
        for (int64_t c : scrambled(chunks)) {
            const int64_t e0 = c * ACCF_CHUNK;
            const AccfSpan s = accf_chunk_span(e0, R, cells);
            assert(s.count >= 1 && s.count <= ACCF_CHUNK + 2 * ACCF_MAX_RADIUS && s.first >= 0 && s.first + s.count <= cells);
            std::vector<u64> lds = poisoned<u64>(ACCF_CHUNK + 2 * ACCF_MAX_RADIUS);
            for (int64_t t = 0; t < s.count; ++t) lds[t] = in[s.first + t];
            for (int64_t e = e0; e < e0 + ACCF_CHUNK && e < cells; ++e) {
                const int64_t i = e % len, base = e - i;
                assert(is_poison(staged[e]));
                staged[e] = accf_line_min(lds.data(), 1, s.first - base, s.count, len, i, R);
                w_staged[e] += 1;
            }
        }
    } else {                                                                                     // off the contiguous axis there is only the direct kernel
        staged = direct;
        w_staged = w_direct;
    }
    all_once(w_staged);
    behind_untouched(staged, cells);
    assert(staged == direct);
    direct.resize(cells);
    return direct;
}

struct Looked { std::vector<int64_t> counters; std::vector<uint8_t> status; std::vector<int32_t> dist2, row; };

static void write_looked(FILE *o, const Looked &l, int64_t n)
{
    behind_untouched(l.status, n); behind_untouched(l.dist2, n); behind_untouched(l.row, n);
    wr(o, l.counters); wr(o, l.status, n); wr(o, l.dist2, n); wr(o, l.row, n);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 14);
    const std::vector<double> g = rd<double>(f, 18);
    const int64_t m = h[0], cap = h[1], min_count = h[2], n_points = h[12], n_coords = h[13];
    const bool use_fraction = h[3] != 0;
    const int R = (int)h[4];
    const AccfBox box = {h[6], h[7], h[8], h[9], h[10], h[11], h[5] != 0 ? 1 : 0};
    const int64_t cells = accf_cells(box), nzo = accf_nz_out(box);
    assert(R >= 1 && R <= ACCF_MAX_RADIUS && cells >= 1 && cells <= ACCF_MAX_CELLS);
    const Map map = read_map(f, m, cap, false, Fills{0, 1000, 0, 0, 0}, MAP_ACC);                 // key 0 = voxel (-2^20, -2^20, -2^20): a site if it were read
    const std::vector<float> points = rd<float>(f, 3 * n_points);
    const std::vector<int32_t> coords = rd<int32_t>(f, 3 * n_coords);

    std::vector<int64_t> counters(ACCF_COUNTERS, 0);
    std::vector<int32_t> dist2 = poisoned<int32_t>(cells + BEHIND), nearest = poisoned<int32_t>(cells + BEHIND);
    if (m == 0) {                                                                                // all -1 and zero counters
        for (int64_t e = 0; e < cells; ++e) dist2[e] = nearest[e] = -1;
    } else {
        const RowTable tab = row_table(map, min_count, use_fraction, g[0]);                     // pass 1 of C5
        AcccMap M;
        M.keys = map.keys.data(); M.acc = map.acc.data(); M.stamps = nullptr; M.rows = tab.rows.data();
        M.capacity = cap; M.m = m; M.kept = tab.kept;
        counters[ACCF_C_ROWS] = tab.kept;

        // the site kernel: one lane per kept row, one writer per cell
        std::vector<u64> grid(cells, ACCF_NONE);
        for (int64_t j = 0; j < tab.kept; ++j) {
            const int64_t cell = accf_site(M, box, j);
            if (cell < 0) continue;
            PCACC_BOUND(cell, cells);
            assert(grid[cell] == ACCF_NONE);
            grid[cell] = accf_pack(0, j);
            assert((grid[cell] >> 32) == 0 && (int64_t)(grid[cell] & 0xffffffffull) == j);
            counters[ACCF_C_SITES] += 1;
        }

        // the passes, uncut in between
        if (!box.planar) grid = pass(grid, cells, 1, nzo, R);
        grid = pass(grid, cells, nzo, box.ny, R);
        grid = pass(grid, cells, box.ny * nzo, box.nx, R);
        for (int64_t e = 0; e < cells; ++e) assert(grid[e] == ACCF_NONE || (grid[e] >> 32) <= 3ull * ACCF_MAX_RADIUS * ACCF_MAX_RADIUS);

        // the cut of the last pass
        std::vector<int> written(cells, 0);
        for (int64_t e = 0; e < cells; ++e) {
            int32_t d2, row;
            const bool near = accf_cut(grid[e], R, &d2, &row);
            assert(near ? (d2 >= 0 && d2 <= R * R && row >= 0 && row < tab.kept) : (d2 == -1 && row == -1));
            assert(is_poison(dist2[e]) && is_poison(nearest[e]));
            dist2[e] = d2; nearest[e] = row;
            written[e] += 1;
            counters[near ? ACCF_C_NEAR : ACCF_C_FAR] += 1;
        }
        all_once(written);
        assert(counters[ACCF_C_NEAR] + counters[ACCF_C_FAR] == cells && counters[ACCF_C_SITES] <= counters[ACCF_C_NEAR]);
    }
    behind_untouched(dist2, cells); behind_untouched(nearest, cells);
    wr(o, counters); wr(o, dist2, cells); wr(o, nearest, cells);

    // the lookup kernel: one lane per row, every output of every row written
    for (int mode = 0; mode < 2; ++mode) {
        const int64_t n = mode == 0 ? n_points : n_coords;
        Looked l = {std::vector<int64_t>(ACCF_LOOKUP_COUNTERS, 0), poisoned<uint8_t>(n + BEHIND), poisoned<int32_t>(n + BEHIND), poisoned<int32_t>(n + BEHIND)};
        for (int64_t i = 0; i < n; ++i) {
            int32_t c[3] = {0, 0, 0};
            bool valid;
            if (mode == 0) {
                unsigned long long key = 0;
                int64_t q[3];
                valid = accum_point(g.data() + 2, points.data() + 3 * i, g[1], &key, q);
                if (valid) accum_unkey(key, c);
            } else {
                c[0] = coords[3 * i]; c[1] = coords[3 * i + 1]; c[2] = coords[3 * i + 2];
                valid = accf_coord_valid(c);
            }
            int32_t d2, row;
            const int status = accf_lookup(valid, c, box, cells, dist2.data(), nearest.data(), &d2, &row);
            assert(((status & ACCF_NEAR) != 0) == (d2 >= 0) && (d2 >= 0) == (row >= 0) && (!(status & ACCF_INSIDE) || (status & ACCF_VALID)));
            assert(is_poison(l.status[i]) && is_poison(l.dist2[i]) && is_poison(l.row[i]));
            l.status[i] = (uint8_t)status; l.dist2[i] = d2; l.row[i] = row;
            l.counters[0] += 1; l.counters[1] += (status & ACCF_VALID) != 0; l.counters[2] += (status & ACCF_INSIDE) != 0; l.counters[3] += (status & ACCF_NEAR) != 0;
        }
        write_looked(o, l, n);
    }
    close_io(f, o);
    return 0;
}
