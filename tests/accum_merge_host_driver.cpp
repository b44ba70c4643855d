// Host build of pcaccumulation_amd/csrc/accum_merge.h (tests/test_accumulate_merge.py): the search of a row of one map in the other, the move of a row of
// either map to its row of the union, and the key and contribution of a re-voxelised row -- the functions the kernels of accum_merge.hip call -- run on
// the CPU with every table index assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps between them (exclusive scan, decide,
// sort, run heads, per-run sums, finish) are the kernels' steps.  The input tables stand at their capacity with poison behind the rows in use that no
// result may depend on; the output tables are poison everywhere before they are written: every destination is written exactly once, keys ascend, and the
// poison behind the rows of the result is untouched (after a TOO_SMALL merge: everywhere).
//   merge   in : i64 0, ma, a_capacity, a_has_pierced, mb, b_capacity, b_has_pierced, out_capacity, b_is_a, add_dropped; map A; map B (unless b_is_a)
//           out: i64 counters[5]; i64 state[8] (before the call: NUM_VOXELS = ma, DROPPED = 100, the rest 7); with STATUS = 0 the map of NEEDED rows
//   regrid  in : i64 1, m, capacity, has_pierced, out_capacity, has_pose, carry_dropped; f64 out_voxel_size, pose[16]; the map
//           out: i64 counters[5]; i64 state[8] (poison before the call); the map of ROWS_OUT rows
//   a map   : see accum_host.h
#include <algorithm>
#include <climits>

#include "accum_merge.h"
#include "accum_host.h"

// the state and counter words of include/pcacc.h (C4, C12) that the steps between the header's functions write
enum { STATE_WORDS = 8, NUM_VOXELS = 0, DROPPED = 1, OK = 0, TOO_SMALL = 1 };
enum { M_STATUS = 0, M_NEEDED = 1, M_SHARED = 2, M_NEW = 3, M_SATURATED = 4 };
enum { G_ROWS_IN = 0, G_ROWS_OUT = 1, G_DROPPED_ROWS = 2, G_DROPPED_POINTS = 3, G_SATURATED = 4 };

// rows past m: a key that would mislead any search that read it, a record that would pass for a real one
static const Fills FILLS = {0, 1000, 1000, 0x7fffffff, 77};

static void run_merge(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const int64_t ma = h[0], mb = h[3], ocap = h[6], add_dropped = h[8];
    const bool same = h[7] != 0;
    const Map A = read_map(f, ma, h[1], h[2] != 0, FILLS);
    const Map B = same ? A : read_map(f, mb, h[4], h[5] != 0, FILLS);
    assert(B.m == mb && ocap >= 1);
    const bool sidecar = A.has_pierced || B.has_pierced;
    Map out = poison_map(ocap, sidecar);
    std::vector<int64_t> counters(5, POISON_ACC), state(STATE_WORDS, 7);
    state[NUM_VOXELS] = ma; state[DROPPED] = 100;
    // M1, M2
    const int64_t nb = mb > 0 ? mb : 1;
    std::vector<int> miss(nb), pos(nb);
    for (int64_t j = 0; j < nb; ++j) {
        int64_t p;
        miss[j] = accm_search(A.keys.data(), ma, B.keys.data(), mb, j, &p);
        assert(p >= 0 && p <= ma && (j < mb || (miss[j] == 0 && p == 0)));
        pos[j] = (int)p;
    }
    const std::vector<int> mrank = scan(miss);
    // M3
    const int64_t fresh = mrank[nb], total = ma + fresh;
    counters[M_NEEDED] = total; counters[M_SHARED] = mb - fresh; counters[M_NEW] = fresh; counters[M_SATURATED] = 0;
    const bool go = total <= ocap;
    counters[M_STATUS] = go ? OK : TOO_SMALL;
    if (go) { state[NUM_VOXELS] = total; state[DROPPED] += add_dropped; }
    int64_t rows = 0;
    if (go) {
        std::vector<int> written(ocap, 0);
        int64_t shared = 0;
        for (int64_t p = 0; p < ma; ++p) {                                       // M4
            const int flags = accm_old_row(A.keys.data(), A.acc.data(), A.stamps.data(), A.p(), A.cap, ma, B.keys.data(), B.acc.data(), B.stamps.data(),
                                           B.p(), B.cap, mb, mrank.data(), nb + 1, p, out.keys.data(), out.acc.data(), out.stamps.data(), out.p(), ocap,
                                           total);
            assert(flags & ACCM_WRITTEN);
            shared += (flags & ACCM_SHARED) != 0;
            counters[M_SATURATED] += (flags & ACCM_SATURATED) != 0;
            const int64_t j = accum_lower_bound(B.keys.data(), mb, A.keys[p]);
            written[accum_merge_dst(p, mrank[j], total)] += 1;
        }
        assert(shared == counters[M_SHARED]);
        for (int64_t j = 0; j < mb; ++j) {                                       // M5
            if (!miss[j]) continue;
            assert(accm_new_row(B.keys.data(), B.acc.data(), B.stamps.data(), B.p(), B.cap, mb, mrank.data(), nb + 1, j, pos[j], out.keys.data(),
                                out.acc.data(), out.stamps.data(), out.p(), ocap, total) == ACCM_WRITTEN);
            written[accum_merge_dst(pos[j], mrank[j], total)] += 1;
        }
        assert_written_once(written, total);
        rows = total;
    }
    assert_poison_from(out, rows);
    wr(o, counters); wr(o, state);
    write_map(o, out, rows);
}

static void run_regrid(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 6);
    const std::vector<double> g = rd<double>(f, 17);
    const int64_t m = h[0], ocap = h[3], carry = h[5];
    const double vs = g[0];
    const double *pose = h[4] ? g.data() + 1 : nullptr;
    const Map A = read_map(f, m, h[1], h[2] != 0, FILLS);
    assert(ocap >= m && ocap >= 1 && vs > 0.0);
    Map out = poison_map(ocap, A.has_pierced);
    std::vector<int64_t> counters(5, 0), state(STATE_WORDS, POISON_ACC);
    double T[16];
    pcacc_pose_seed(T, pose);
    // G1
    std::vector<std::pair<u64, int> > pairs(m);
    for (int64_t i = 0; i < m; ++i) {
        u64 key;
        int64_t term[ACC_FIELDS], count;
        if (!accg_row(A.acc.data(), A.cap, m, i, T, vs, &key, term, &count)) {
            key = ACC_INVALID_KEY;
            counters[G_DROPPED_ROWS] += 1;
            counters[G_DROPPED_POINTS] += count > 0 ? count : 0;
        } else {
            assert(key != ACC_INVALID_KEY && term[0] == count && count > 0);
            for (int a = 2; a < ACC_FIELDS; ++a) assert(term[a] > -((int64_t)1 << 62) && term[a] < ((int64_t)1 << 62));
        }
        pairs[i] = std::make_pair(key, (int)i);
    }
    // G2, G3
    std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<u64, int> &a, const std::pair<u64, int> &b) { return a.first < b.first; });
    std::vector<int> head(m);
    for (int64_t i = 0; i < m; ++i) head[i] = (pairs[i].first != ACC_INVALID_KEY && (i == 0 || pairs[i - 1].first != pairs[i].first)) ? 1 : 0;
    const std::vector<int> vox = scan(head);
    const int64_t runs = vox[m];
    assert(runs <= m);
    // G4
    std::vector<int64_t> rays(runs, 0);
    std::vector<int> heads_written(runs, 0);
    for (int64_t e = 0; e < runs; ++e) {
        for (int c = 0; c < ACC_FIELDS; ++c) out.acc[accum_field(c, e, ocap)] = 0;
        out.stamps[e] = INT32_MAX;
        out.stamps[ocap + e] = INT32_MIN;
    }
    // G5
    for (int64_t i = 0; i < m; ++i) {
        const u64 key = pairs[i].first;
        const int64_t row = accum_point_index(pairs[i].second, m);
        assert(row >= 0);
        if (key == ACC_INVALID_KEY) continue;
        const int64_t r = accum_run_index(vox[i], head[i], runs);
        assert(r >= 0);
        u64 k2;
        int64_t term[ACC_FIELDS], count;
        assert(accg_row(A.acc.data(), A.cap, m, row, T, vs, &k2, term, &count) && k2 == key);
        PCACC_BOUND(r, ocap);
        if (head[i]) { out.keys[r] = key; heads_written[r] += 1; }
        for (int c = 0; c < ACC_FIELDS; ++c) out.acc[accum_field(c, r, ocap)] += term[c];
        PCACC_BOUND(row, A.cap);
        out.stamps[r] = std::min(out.stamps[r], A.stamps[row]);
        out.stamps[ocap + r] = std::max(out.stamps[ocap + r], A.stamps[A.cap + row]);
        if (A.has_pierced) rays[r] += A.pierced[row];
    }
    // G6
    for (int64_t e = 0; e < runs; ++e) {
        assert(heads_written[e] == 1);
        if (A.has_pierced) {
            int sat;
            out.pierced[e] = accm_pierced(rays[e], &sat);
            counters[G_SATURATED] += sat;
        }
    }
    counters[G_ROWS_IN] = m; counters[G_ROWS_OUT] = runs;
    for (int k = 0; k < STATE_WORDS; ++k) state[k] = 0;
    state[NUM_VOXELS] = runs; state[DROPPED] = carry + counters[G_DROPPED_POINTS];
    assert_poison_from(out, runs);
    wr(o, counters); wr(o, state);
    write_map(o, out, runs);
}

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const int64_t mode = rd<int64_t>(f, 1)[0];
    assert(mode == 0 || mode == 1);
    if (mode == 0) run_merge(f, o); else run_regrid(f, o);
    close_io(f, o);
    return 0;
}
