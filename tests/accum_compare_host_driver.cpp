// Host build of pcaccumulation_amd/csrc/accum_compare.h (tests/test_accumulate_compare.py): the answer for one row of one map against the other map,
// its store, and the select flag of a map row -- the functions the kernels of accum_compare.hip call -- run on the CPU with every table index
// assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps between them (keep flags, exclusive scan, row table, move, counters,
// state) are the kernels' steps.  The input tables stand at their capacity with poison behind the rows in use that no result may depend on; the output
// columns and tables are poison everywhere before they are written: every output row is written exactly once and the poison behind the rows of the
// result is untouched (after a refused select: everywhere, the state words included).
//   compare  in : i64 0, ma, a_capacity, a_has_pierced, mb, b_capacity, b_has_pierced, b_is_a, min_count, use_fraction; f64 max_moving_fraction,
//                 max_distance; map A; map B (unless b_is_a)
//            out: i64 counters[12]; side A then side B, KEPT rows each: u8 status, i32 same_row, i32 row, f64 distance, i32 pierced
//   select   in : i64 1, m, capacity, has_pierced, out_capacity, min_count, use_fraction, mask_rows, invert; f64 max_moving_fraction; the map;
//                 u8 mask[mask_rows]
//            out: i64 counters[4]; i64 state[8] (poison before the call); with STATUS = 0 the map of SELECTED rows
//   a map   : see accum_host.h
#include <cstdlib>

#include "accum_compare.h"
#include "accum_host.h"

enum { STATE_WORDS = 8, NUM_VOXELS = 0 };                                        // include/pcacc.h (C4)

// rows past m: a key that would mislead any search that read it, a record that would pass for a real one
static const Fills FILLS = {0, 1000, 1000, 0x7fffffff, 77};

// a map and its row table under the filter
struct Side : Map {
    RowTable tab;
};

static Side read_side(FILE *f, int64_t m, int64_t cap, bool has_pierced, int64_t min_count, bool use_fraction, double fraction)
{
    Side s;
    static_cast<Map &>(s) = read_map(f, m, cap, has_pierced, FILLS);
    s.tab = row_table(s, min_count, use_fraction, fraction);
    return s;
}

static AccdMap view(const Side &t)
{
    AccdMap v;
    v.keys = t.m ? t.keys.data() : nullptr;                                      // a side without rows: nothing of it may be addressed
    v.acc = t.m ? t.acc.data() : nullptr;
    v.pierced = t.m ? t.p() : nullptr;
    v.dst = t.m ? t.tab.dst.data() : nullptr;
    v.capacity = t.cap; v.m = t.m; v.kept = t.tab.kept;
    return v;
}

static void compare_side(const Side &own, const Side &other, double max_d2, int64_t *counters, FILE *o)
{
    const int64_t rows = own.m > 0 ? own.m : 1, kept = own.tab.kept;
    std::vector<uint8_t> status(rows, POISON_U8);
    std::vector<int32_t> same_row(rows, POISON_I32), row(rows, POISON_I32), pierced(rows, POISON_I32);
    std::vector<double> distance(rows, POISON_F64);
    std::vector<int> written(rows, 0);
    const AccdOut out = {status.data(), same_row.data(), row.data(), pierced.data(), distance.data()};
    const AccdMap a = view(own), b = view(other);
    for (int k = 0; k < ACCD_SIDE_COUNTERS; ++k) counters[k] = 0;
    counters[ACCD_C_ROWS] = own.m;
    counters[ACCD_C_KEPT] = kept;
    for (int64_t j = 0; j < kept; ++j) {
        const int64_t i = own.tab.rows[j];
        assert(i >= 0 && i < own.m && own.tab.dst[i] == j);
        AccdRecord r;
        assert(accd_row(a, b, i, max_d2, &r));
        assert(accd_store(out, j, kept, own.m, r));
        written[j] += 1;
        assert((r.status & ~(ACCD_SAME | ACCD_HELD | ACCD_NEAR)) == 0 && (!(r.status & ACCD_SAME) || (r.status & ACCD_HELD)));
        assert(((r.status & ACCD_SAME) != 0) == (r.same_row >= 0) && ((r.status & ACCD_NEAR) != 0) == (r.row >= 0));
        assert(r.same_row < other.tab.kept && r.row < other.tab.kept &&((r.status & ACCD_NEAR) ? r.distance * r.distance <= max_d2 * (1.0 + 1e-12) : r.distance > 1e300));
        counters[ACCD_C_SAME] += (r.status & ACCD_SAME) != 0;
        counters[ACCD_C_HELD] += (r.status & ACCD_HELD) != 0;
        counters[ACCD_C_NEAR] += (r.status & ACCD_NEAR) != 0;
        counters[ACCD_C_ONLY] += (r.status & (ACCD_SAME | ACCD_NEAR)) == 0;
    }
    const AccdRecord r = {0.0, -1, -1, 0, 0};                                    // no row of the side, a row behind the kept ones: nothing is written
    assert(!accd_store(out, kept, kept, own.m, r) && !accd_store(out, -1, kept, own.m, r));
    assert_written_once(written, kept);
    for (int64_t j = kept; j < rows; ++j)
        assert(status[j] == POISON_U8 && same_row[j] == POISON_I32 && row[j] == POISON_I32 && pierced[j] == POISON_I32 && distance[j] == POISON_F64);
    wr(o, status, kept); wr(o, same_row, kept); wr(o, row, kept); wr(o, distance, kept); wr(o, pierced, kept);
}

static void run_compare(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const std::vector<double> g = rd<double>(f, 2);
    const bool same = h[6] != 0, use_fraction = h[8] != 0;
    const int64_t min_count = h[7];
    assert(min_count >= 1 && g[1] > 0.0);
    const Side A = read_side(f, h[0], h[1], h[2] != 0, min_count, use_fraction, g[0]);
    const Side B = same ? A : read_side(f, h[3], h[4], h[5] != 0, min_count, use_fraction, g[0]);
    assert(B.m == h[3]);
    const double max_d2 = g[1] * g[1];
    std::vector<int64_t> counters(ACCD_COUNTERS, POISON_ACC);
    char *side_a = nullptr, *side_b = nullptr;
    size_t na = 0, nb = 0;
    FILE *fa = open_memstream(&side_a, &na), *fb = open_memstream(&side_b, &nb);
    assert(fa && fb);
    compare_side(A, B, max_d2, counters.data(), fa);
    compare_side(B, A, max_d2, counters.data() + ACCD_SIDE_COUNTERS, fb);
    fclose(fa); fclose(fb);
    wr(o, counters, counters.size());
    if (na) assert(fwrite(side_a, 1, na, o) == na);
    if (nb) assert(fwrite(side_b, 1, nb, o) == nb);
    free(side_a); free(side_b);
}

static void run_select(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 8);
    const std::vector<double> g = rd<double>(f, 1);
    const int64_t m = h[0], ocap = h[3], min_count = h[4], mask_rows = h[6];
    const int invert = h[7] != 0;
    assert(ocap >= m && ocap >= 1 && min_count >= 1);
    const Side A = read_side(f, m, h[1], h[2] != 0, min_count, h[5] != 0, g[0]);
    std::vector<uint8_t> mask = rd<uint8_t>(f, mask_rows);
    mask.push_back(1);                                                           // poison behind the mask: an entry that would select
    Map out = poison_map(ocap, A.has_pierced);
    std::vector<int64_t> counters(ACCS_COUNTERS, POISON_ACC), state(STATE_WORDS, POISON_ACC);
    const int status = accs_status(A.tab.kept, mask_rows);
    const uint8_t *mask_ptr = status == ACCS_OK ? mask.data() : nullptr;         // BAD_MASK: no mask entry may be addressed
    const int *dst = A.tab.dst.data();
    std::vector<int> flag(m);
    for (int64_t i = 0; i < m; ++i) flag[i] = accs_selected(dst, m, mask_ptr, mask_rows, status, invert, i);
    const std::vector<int> spos = scan(flag);
    assert(accs_selected(dst, m, mask_ptr, mask_rows, status, invert, m) == 0 && accs_selected(dst, m, mask_ptr, mask_rows, status, invert, -1) == 0);
    const int64_t selected = status == ACCS_OK ? spos[m] : 0;
    assert(status == ACCS_OK || spos[m] == 0);
    std::vector<int> written(ocap, 0);
    if (status == ACCS_OK)
        for (int64_t i = 0; i < m; ++i) {
            if (!flag[i]) continue;
            const int64_t d = accum_merge_dst(spos[i], 0, selected);
            assert(accr_move_row(A.keys.data(), A.acc.data(), A.stamps.data(), A.p(), A.cap, m, i, out.keys.data(), out.acc.data(), out.stamps.data(),
                                 out.p(), ocap, selected, d));
            written[d] += 1;
        }
    counters[ACCS_C_STATUS] = status; counters[ACCS_C_ROWS] = m; counters[ACCS_C_KEPT] = A.tab.kept; counters[ACCS_C_SELECTED] = selected;
    if (status == ACCS_OK) {
        for (int k = 0; k < STATE_WORDS; ++k) state[k] = 0;
        state[NUM_VOXELS] = selected;
    }
    assert_written_once(written, selected);
    assert_poison_from(out, selected);
    wr(o, counters); wr(o, state);
    write_map(o, out, selected);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const int64_t mode = rd<int64_t>(f, 1)[0];
    assert(mode == 0 || mode == 1);
    if (mode == 0) run_compare(f, o); else run_select(f, o);
    close_io(f, o);
    return 0;
}
