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
//   a map   : i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; i32 pierced[m] (with a sidecar)
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "accum_compare.h"

typedef unsigned long long u64;

#define POISON_KEY 0x5a5a5a5a5a5a5a5aull
#define POISON_ACC 0x5b5b5b5b5b5b5b5bll
#define POISON_I32 0x5c5c5c5c
#define POISON_U8 0x5d
#define POISON_F64 -12345.678

enum { STATE_WORDS = 8, NUM_VOXELS = 0 };                                        // include/pcacc.h (C4)

template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n) assert(fread(v.data(), sizeof(T), n, f) == n);
    return v;
}

template <class T> static void wr(FILE *f, const std::vector<T> &v, size_t n)
{
    assert(n <= v.size());
    if (n) assert(fwrite(v.data(), sizeof(T), n, f) == n);
}

struct Map {
    int64_t m, cap;
    bool has_pierced;
    std::vector<u64> keys;
    std::vector<int64_t> acc;
    std::vector<int32_t> stamps, pierced;
    std::vector<int> dst, rows;                                                  // the row table under the filter
    int64_t kept;
    const int32_t *p() const { return has_pierced ? pierced.data() : nullptr; }
    int32_t *p() { return has_pierced ? pierced.data() : nullptr; }
};

// rows past m: a key that would mislead any search that read it, a record that would pass for a real one
static Map read_map(FILE *f, int64_t m, int64_t cap, bool has_pierced)
{
    assert(m >= 0 && cap >= m && cap >= 1);
    Map t;
    t.m = m; t.cap = cap; t.has_pierced = has_pierced; t.kept = 0;
    t.keys.assign(cap, 0);
    t.acc.assign((size_t)ACC_FIELDS * cap, 1000);
    t.stamps.assign(2 * cap, 0x7fffffff);
    t.pierced.assign(has_pierced ? cap : 0, 77);
    const std::vector<int64_t> k = rd<int64_t>(f, m), a = rd<int64_t>(f, (size_t)ACC_FIELDS * m);
    const std::vector<int32_t> s = rd<int32_t>(f, 2 * m), p = rd<int32_t>(f, has_pierced ? m : 0);
    for (int64_t i = 0; i < m; ++i) {
        t.keys[i] = (u64)k[i];
        assert(i == 0 || t.keys[i - 1] < t.keys[i]);
        for (int c = 0; c < ACC_FIELDS; ++c) t.acc[(size_t)c * cap + i] = a[(size_t)c * m + i];
        t.stamps[i] = s[i];
        t.stamps[cap + i] = s[m + i];
        if (has_pierced) t.pierced[i] = p[i];
    }
    return t;
}

// pass 1 of C5: keep flags (extract's predicate), exclusive scan, dst and its inverse
static void row_table(Map &t, int64_t min_count, bool use_fraction, double fraction)
{
    t.dst.assign(t.m, -1);
    t.rows.clear();
    std::vector<int> keep(t.m), kpos(t.m + 1, 0);
    for (int64_t i = 0; i < t.m; ++i) {
        keep[i] = accum_keep(t.acc[accum_field(0, i, t.cap)], t.acc[accum_field(1, i, t.cap)], min_count, use_fraction, fraction) ? 1 : 0;
        kpos[i + 1] = kpos[i] + keep[i];
    }
    t.kept = kpos[t.m];
    t.rows.assign(t.kept, -1);
    for (int64_t i = 0; i < t.m; ++i) {
        if (!keep[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, t.kept);
        assert(d >= 0);
        t.dst[i] = (int)d;
        t.rows[d] = (int)i;
    }
}

static AccdMap view(const Map &t)
{
    AccdMap v;
    v.keys = t.m ? t.keys.data() : nullptr;                                      // a side without rows: nothing of it may be addressed
    v.acc = t.m ? t.acc.data() : nullptr;
    v.pierced = t.m ? t.p() : nullptr;
    v.dst = t.m ? t.dst.data() : nullptr;
    v.capacity = t.cap; v.m = t.m; v.kept = t.kept;
    return v;
}

static void compare_side(const Map &own, const Map &other, double max_d2, int64_t *counters, FILE *o)
{
    const int64_t rows = own.m > 0 ? own.m : 1;
    std::vector<uint8_t> status(rows, POISON_U8);
    std::vector<int32_t> same_row(rows, POISON_I32), row(rows, POISON_I32), pierced(rows, POISON_I32);
    std::vector<double> distance(rows, POISON_F64);
    std::vector<int> written(rows, 0);
    const AccdOut out = {status.data(), same_row.data(), row.data(), pierced.data(), distance.data()};
    const AccdMap a = view(own), b = view(other);
    for (int k = 0; k < ACCD_SIDE_COUNTERS; ++k) counters[k] = 0;
    counters[ACCD_C_ROWS] = own.m;
    counters[ACCD_C_KEPT] = own.kept;
    for (int64_t j = 0; j < own.kept; ++j) {
        const int64_t i = own.rows[j];
        assert(i >= 0 && i < own.m && own.dst[i] == j);
        AccdRecord r;
        assert(accd_row(a, b, i, max_d2, &r));
        assert(accd_store(out, j, own.kept, own.m, r));
        written[j] += 1;
        assert((r.status & ~(ACCD_SAME | ACCD_HELD | ACCD_NEAR)) == 0 && (!(r.status & ACCD_SAME) || (r.status & ACCD_HELD)));
        assert(((r.status & ACCD_SAME) != 0) == (r.same_row >= 0) && ((r.status & ACCD_NEAR) != 0) == (r.row >= 0));
        assert(r.same_row < other.kept && r.row < other.kept && ((r.status & ACCD_NEAR) ? r.distance * r.distance <= max_d2 * (1.0 + 1e-12) : r.distance > 1e300));
        counters[ACCD_C_SAME] += (r.status & ACCD_SAME) != 0;
        counters[ACCD_C_HELD] += (r.status & ACCD_HELD) != 0;
        counters[ACCD_C_NEAR] += (r.status & ACCD_NEAR) != 0;
        counters[ACCD_C_ONLY] += (r.status & (ACCD_SAME | ACCD_NEAR)) == 0;
    }
    const AccdRecord r = {0.0, -1, -1, 0, 0};                                    // no row of the side, a row behind the kept ones: nothing is written
    assert(!accd_store(out, own.kept, own.kept, own.m, r) && !accd_store(out, -1, own.kept, own.m, r));
    for (int64_t j = 0; j < rows; ++j) {
        assert(written[j] == (j < own.kept ? 1 : 0));
        if (j >= own.kept)
            assert(status[j] == POISON_U8 && same_row[j] == POISON_I32 && row[j] == POISON_I32 && pierced[j] == POISON_I32 && distance[j] == POISON_F64);
    }
    wr(o, status, own.kept); wr(o, same_row, own.kept); wr(o, row, own.kept); wr(o, distance, own.kept); wr(o, pierced, own.kept);
}

static void run_compare(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const std::vector<double> g = rd<double>(f, 2);
    const bool same = h[6] != 0, use_fraction = h[8] != 0;
    const int64_t min_count = h[7];
    assert(min_count >= 1 && g[1] > 0.0);
    Map A = read_map(f, h[0], h[1], h[2] != 0);
    row_table(A, min_count, use_fraction, g[0]);
    Map B = same ? A : read_map(f, h[3], h[4], h[5] != 0);
    if (!same) row_table(B, min_count, use_fraction, g[0]);
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
    Map A = read_map(f, m, h[1], h[2] != 0);
    std::vector<uint8_t> mask = rd<uint8_t>(f, mask_rows);
    mask.push_back(1);                                                           // poison behind the mask: an entry that would select
    assert(ocap >= m && ocap >= 1 && min_count >= 1);
    row_table(A, min_count, h[5] != 0, g[0]);
    Map out;
    out.m = 0; out.cap = ocap; out.has_pierced = A.has_pierced; out.kept = 0;
    out.keys.assign(ocap, POISON_KEY);
    out.acc.assign((size_t)ACC_FIELDS * ocap, POISON_ACC);
    out.stamps.assign(2 * ocap, POISON_I32);
    out.pierced.assign(A.has_pierced ? ocap : 0, POISON_I32);
    std::vector<int64_t> counters(ACCS_COUNTERS, POISON_ACC), state(STATE_WORDS, POISON_ACC);
    const int status = accs_status(A.kept, mask_rows);
    const uint8_t *mask_ptr = status == ACCS_OK ? mask.data() : nullptr;         // BAD_MASK: no mask entry may be addressed
    std::vector<int> flag(m), spos(m + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        flag[i] = accs_selected(A.dst.data(), m, mask_ptr, mask_rows, status, invert, i);
        spos[i + 1] = spos[i] + flag[i];
    }
    assert(accs_selected(A.dst.data(), m, mask_ptr, mask_rows, status, invert, m) == 0 && accs_selected(A.dst.data(), m, mask_ptr, mask_rows, status, invert, -1) == 0);
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
    counters[ACCS_C_STATUS] = status; counters[ACCS_C_ROWS] = m; counters[ACCS_C_KEPT] = A.kept; counters[ACCS_C_SELECTED] = selected;
    if (status == ACCS_OK) {
        for (int k = 0; k < STATE_WORDS; ++k) state[k] = 0;
        state[NUM_VOXELS] = selected;
    }
    for (int64_t d = 0; d < ocap; ++d) {
        assert(written[d] == (d < selected ? 1 : 0));
        assert(d == 0 || d >= selected || out.keys[d - 1] < out.keys[d]);
        if (d < selected) continue;
        assert(out.keys[d] == POISON_KEY && out.stamps[d] == POISON_I32 && out.stamps[ocap + d] == POISON_I32);
        for (int c = 0; c < ACC_FIELDS; ++c) assert(out.acc[(size_t)c * ocap + d] == POISON_ACC);
        if (out.has_pierced) assert(out.pierced[d] == POISON_I32);
    }
    wr(o, counters, counters.size()); wr(o, state, state.size());
    std::vector<int64_t> k64(selected), a64((size_t)ACC_FIELDS * selected);
    std::vector<int32_t> s32(2 * selected), p32(out.has_pierced ? selected : 0);
    for (int64_t d = 0; d < selected; ++d) {
        k64[d] = (int64_t)out.keys[d];
        for (int c = 0; c < ACC_FIELDS; ++c) a64[(size_t)c * selected + d] = out.acc[(size_t)c * ocap + d];
        s32[d] = out.stamps[d];
        s32[selected + d] = out.stamps[ocap + d];
        if (out.has_pierced) p32[d] = out.pierced[d];
    }
    wr(o, k64, k64.size()); wr(o, a64, a64.size()); wr(o, s32, s32.size()); wr(o, p32, p32.size());
}

int main(int argc, char **argv)
{
    assert(argc == 3);
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    assert(f && o);
    const int64_t mode = rd<int64_t>(f, 1)[0];
    assert(mode == 0 || mode == 1);
    if (mode == 0) run_compare(f, o); else run_select(f, o);
    fclose(o);
    fclose(f);
    return 0;
}
