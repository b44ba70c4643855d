// Host build of pcaccumulation_amd/csrc/accum_observe_merge.h (tests/test_accumulate_observe_merge.py): ONE pcacc_accum_observed_merge or ONE
// pcacc_accum_observed_regrid, stage by stage as accum_observe_merge.hip runs them, on the CPU with every index assert-checked (-DPCACC_HOST_CHECK),
// before anything runs on a GPU.
// The input tables stand at their capacity with misleading rows behind the rows in use; the output table and the output state are poisoned first: every
// destination row is written exactly once, keys ascend, what lies behind the last row is asserted untouched, and a call that is refused is asserted to
// have left the output (and, for a merge, the state) as it was.
//   merge  in : i64 0, ma, a_capacity, mb, b_capacity, out_capacity, same (1: B is A -- the same tables and state words), 0;
//               A: i64 keys[ma]; i64 rays[ma]; i32 stamps[2][ma]; i64 state[16];  B likewise, unless same
//          out: i64 counters[4]; i64 state[16]; i64 rows (0 unless OK); i64 keys[rows]; i64 rays[rows]; i32 stamps[2][rows]
//   regrid in : i64 1, m, in_capacity, out_capacity, has_pose, 0, 0, 0; f64 in_voxel_size, out_voxel_size; f64 pose[16];
//               i64 keys[m]; i64 rays[m]; i32 stamps[2][m]; i64 in_state[16]
//          out: i64 counters[3]; i64 out_state[16] (poison where not written); i64 rows; i64 keys[rows]; i64 rays[rows]; i32 stamps[2][rows]
#include <algorithm>

#include "accum_observe_merge.h"
#include "accum_host.h"

struct Table {
    int64_t m, cap;
    std::vector<u64> keys;
    std::vector<int64_t> rays;
    std::vector<int32_t> stamps;                                                 // [2][cap]
};

// m rows from the file into tables of `cap` rows; the rows behind m: a key that would mislead any search that read it, a ray count and stamps no
// result may show.
static Table read_table(FILE *f, int64_t m, int64_t cap)
{
    assert(m >= 0 && cap >= m);
    const int64_t room = std::max<int64_t>(cap, 1);
    Table t;
    t.m = m; t.cap = cap;
    t.keys.assign(room, 0);
    t.rays.assign(room, 77);
    t.stamps.assign(2 * room, -7);
    const std::vector<int64_t> k = rd<int64_t>(f, m), r = rd<int64_t>(f, m);
    const std::vector<int32_t> s = rd<int32_t>(f, 2 * m);
    for (int64_t i = 0; i < m; ++i) {
        t.keys[i] = (u64)k[i]; t.rays[i] = r[i]; t.stamps[i] = s[i]; t.stamps[cap + i] = s[m + i];
        assert(i == 0 || t.keys[i - 1] < t.keys[i]);
    }
    return t;
}

static Table poison_table(int64_t cap)
{
    Table t;
    t.m = 0; t.cap = cap;
    t.keys.assign(std::max<int64_t>(cap, 1), POISON_KEY);
    t.rays.assign(std::max<int64_t>(cap, 1), POISON_ACC);
    t.stamps.assign(2 * std::max<int64_t>(cap, 1), POISON_I32);
    return t;
}

static void assert_table_poison_from(const Table &t, int64_t row)
{
    for (int64_t d = row; d < t.cap; ++d)
        assert(t.keys[d] == POISON_KEY && t.rays[d] == POISON_ACC && t.stamps[d] == POISON_I32 && t.stamps[t.cap + d] == POISON_I32);
}

static void write_table(FILE *o, const Table &t, int64_t rows)
{
    std::vector<int64_t> k64(rows), r64(rows);
    std::vector<int32_t> s32(2 * rows);
    for (int64_t d = 0; d < rows; ++d) {
        assert(d == 0 || t.keys[d - 1] < t.keys[d]);
        k64[d] = (int64_t)t.keys[d]; r64[d] = t.rays[d]; s32[d] = t.stamps[d]; s32[rows + d] = t.stamps[t.cap + d];
    }
    wr1(o, rows);
    wr(o, k64); wr(o, r64); wr(o, s32);
}

static void merge(FILE *f, FILE *o, const std::vector<int64_t> &h)
{
    const int64_t ma = h[1], a_cap = h[2], out_cap = h[5];
    const bool same = h[6] != 0;
    const Table A = read_table(f, ma, a_cap);
    std::vector<int64_t> state = rd<int64_t>(f, ACCOM_STATE_WORDS);
    const Table B_own = same ? Table() : read_table(f, h[3], h[4]);
    const std::vector<int64_t> b_own_state = same ? std::vector<int64_t>() : rd<int64_t>(f, ACCOM_STATE_WORDS);
    const Table &B = same ? A : B_own;
    const int64_t *b_state = same ? state.data() : b_own_state.data();            // the same words, as the device call has them
    const int64_t mb = B.m, b_cap = B.cap;
    assert(ma <= a_cap && mb <= b_cap && out_cap >= 0);
    const std::vector<int64_t> state_before(state);
    if (ma == 0 && mb == 0) {                                                    // the zero counters, and nothing else
        wr(o, std::vector<int64_t>(4, 0));
        wr(o, state);
        write_table(o, poison_table(out_cap), 0);
        return;
    }

    // M0 begin
    const bool bad = !accom_state_fits(state.data(), ma, b_state, mb);

    // M1 search: with state words that do not fit, no table is addressed
    const int64_t nb = mb > 0 ? mb : 1;
    std::vector<int> miss(nb, 0), pos(nb, 0);
    for (int64_t j = 0; j < nb && !bad; ++j) {
        int64_t p;
        miss[j] = accm_search(A.keys.data(), ma, B.keys.data(), mb, j, &p);
        assert(p >= 0 && p <= ma);
        pos[j] = (int)p;
    }

    // M2 scan, M3 decide
    const std::vector<int> mrank = scan(miss);
    std::vector<int64_t> counters(4, POISON_ACC);
    const int status = accom_decide(bad, ma, mb, mrank[nb], out_cap, b_state, state.data(), counters.data());
    const int64_t total = ma + mrank[nb];
    assert(counters[ACCOM_C_STATUS] == status);
    if (status != ACCO_OK) assert(state == state_before);                        // a refusal writes no state word
    if (status == ACCO_OK) assert(counters[ACCOM_C_NEEDED] == total && counters[ACCOM_C_SHARED] + counters[ACCOM_C_NEW] == mb);

    // M4, M5 into a poisoned table
    Table out = poison_table(out_cap);
    if (status == ACCO_OK) {
        std::vector<int> written(out_cap, 0);
        int64_t shared_rows = 0;
        for (int64_t p = 0; p < ma; ++p) {
            int shared;
            const int64_t d = accom_old_row(A.keys.data(), A.rays.data(), A.stamps.data(), a_cap, ma, B.keys.data(), B.rays.data(), B.stamps.data(), b_cap, mb,
                                            mrank.data(), nb + 1, p, out.keys.data(), out.rays.data(), out.stamps.data(), out_cap, total, &shared);
            assert(d >= 0 && d < total);
            ++written[d];
            shared_rows += shared;
        }
        for (int64_t j = 0; j < mb; ++j) {
            if (!miss[j]) continue;
            const int64_t d = accom_new_row(B.keys.data(), B.rays.data(), B.stamps.data(), b_cap, mb, mrank.data(), nb + 1, j, pos[j], out.keys.data(),
                                            out.rays.data(), out.stamps.data(), out_cap, total);
            assert(d >= 0 && d < total);
            ++written[d];
        }
        assert_written_once(written, total);
        assert(shared_rows == counters[ACCOM_C_SHARED]);
        for (int64_t d = 1; d < total; ++d) assert(out.keys[d - 1] < out.keys[d]);
    }
    assert_table_poison_from(out, status == ACCO_OK ? total : 0);
    wr(o, counters);
    wr(o, state);
    write_table(o, out, status == ACCO_OK ? total : 0);
}

static void regrid(FILE *f, FILE *o, const std::vector<int64_t> &h)
{
    const int64_t m = h[1], in_cap = h[2], out_cap = h[3];
    const std::vector<double> g = rd<double>(f, 2), pose = rd<double>(f, 16);
    const double in_vs = g[0], out_vs = g[1];
    assert(m >= 0 && in_cap >= m && out_cap >= m && in_vs > 0.0 && out_vs > 0.0);
    const Table in = read_table(f, m, in_cap);
    const std::vector<int64_t> in_state = rd<int64_t>(f, ACCOM_STATE_WORDS);
    double T[16];
    pcacc_pose_seed(T, h[4] ? pose.data() : nullptr);
    std::vector<int64_t> counters(3, 0), out_state(ACCOM_STATE_WORDS, POISON_ACC);

    // G0 begin
    const bool bad = in_state[ACCOM_NUM_VOXELS] != m;

    // G1 keys: with state words that do not fit, every key is the invalid one and no table is addressed
    std::vector<std::pair<u64, int>> pairs(m);
    for (int64_t i = 0; i < m; ++i) {
        u64 key = ACC_INVALID_KEY;
        if (!bad && !accog_row(in.keys.data(), in_cap, m, i, T, in_vs, out_vs, &key)) {
            key = ACC_INVALID_KEY;
            ++counters[ACCOG_C_DROPPED_ROWS];
        }
        pairs[i] = std::make_pair(key, (int)i);
    }

    // G2 sort
    std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<u64, int> &a, const std::pair<u64, int> &b) { return a.first < b.first; });
    std::vector<u64> sorted(std::max<int64_t>(m, 1), POISON_KEY);
    std::vector<int> idx(std::max<int64_t>(m, 1), -1);
    for (int64_t i = 0; i < m; ++i) { sorted[i] = pairs[i].first; idx[i] = pairs[i].second; }

    // G3 heads + scan
    std::vector<int> head(m);
    for (int64_t i = 0; i < m; ++i) head[i] = accog_head(sorted.data(), i, m);
    const std::vector<int> vox = scan(head);
    const int64_t runs = vox[m];
    assert(runs >= 0 && runs <= m && (!bad || runs == 0));

    // G4 clear, G5 reduce into a poisoned table
    Table out = poison_table(out_cap);
    for (int64_t e = 0; e < runs; ++e) { PCACC_BOUND(e, out_cap); out.rays[e] = 0; out.stamps[e] = INT32_MAX; out.stamps[out_cap + e] = INT32_MIN; }
    std::vector<int> keyed(out_cap, 0), sources(out_cap, 0);
    int64_t folded = 0;
    for (int64_t i = 0; i < m; ++i) {
        int64_t row;
        const int64_t run = accog_position(sorted.data(), idx.data(), head.data(), vox.data(), m, runs, i, &row);
        if (run < 0) { assert(sorted[i] == ACC_INVALID_KEY); continue; }
        PCACC_BOUND(run, runs);
        PCACC_BOUND(run, out_cap);
        PCACC_BOUND(row, in_cap);
        if (head[i]) { out.keys[run] = sorted[i]; ++keyed[run]; }
        accog_fold(&out.rays[run], &out.stamps[run], &out.stamps[out_cap + run], in.rays[row], in.stamps[row], in.stamps[in_cap + row]);
        ++sources[run];
        ++folded;
    }
    assert_written_once(keyed, runs);
    for (int64_t e = 0; e < runs; ++e) assert(sources[e] >= 1 && (e == 0 || out.keys[e - 1] < out.keys[e]));
    assert(bad || folded + counters[ACCOG_C_DROPPED_ROWS] == m);
    assert_table_poison_from(out, runs);

    // G6 finish
    if (bad) out_state[ACCOM_STATUS] = ACCO_BAD_STATE;
    else {
        counters[ACCOG_C_ROWS_IN] = m;
        counters[ACCOG_C_ROWS_OUT] = runs;
        accog_state(in_state.data(), runs, out_state.data());
    }
    wr(o, counters);
    wr(o, out_state);
    write_table(o, out, runs);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 8);
    if (h[0] == 0) merge(f, o, h); else regrid(f, o, h);
    close_io(f, o);
    return 0;
}
