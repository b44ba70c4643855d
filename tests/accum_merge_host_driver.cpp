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
//   a map   : i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; i32 pierced[m] (with a sidecar)
#include <algorithm>
#include <cassert>
#include <climits>
#include <cstdio>
#include <vector>

#include "accum_merge.h"

typedef unsigned long long u64;

#define POISON_KEY 0x5a5a5a5a5a5a5a5aull
#define POISON_ACC 0x5b5b5b5b5b5b5b5bll
#define POISON_I32 0x5c5c5c5c

// the state and counter words of include/pcacc.h (C4, C12) that the steps between the header's functions write
enum { STATE_WORDS = 8, NUM_VOXELS = 0, DROPPED = 1, OK = 0, TOO_SMALL = 1 };
enum { M_STATUS = 0, M_NEEDED = 1, M_SHARED = 2, M_NEW = 3, M_SATURATED = 4 };
enum { G_ROWS_IN = 0, G_ROWS_OUT = 1, G_DROPPED_ROWS = 2, G_DROPPED_POINTS = 3, G_SATURATED = 4 };

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

struct Map {
    int64_t m, cap;
    bool has_pierced;
    std::vector<u64> keys;
    std::vector<int64_t> acc;
    std::vector<int32_t> stamps, pierced;
    const int32_t *p() const { return has_pierced ? pierced.data() : nullptr; }
    int32_t *p() { return has_pierced ? pierced.data() : nullptr; }
};

// rows past m: a key that would mislead any search that read it, a record that would pass for a real one
static Map read_map(FILE *f, int64_t m, int64_t cap, bool has_pierced)
{
    assert(m >= 0 && cap >= m && cap >= 1);
    Map t;
    t.m = m; t.cap = cap; t.has_pierced = has_pierced;
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

static Map poison_map(int64_t cap, bool has_pierced)
{
    Map t;
    t.m = 0; t.cap = cap; t.has_pierced = has_pierced;
    t.keys.assign(cap, POISON_KEY);
    t.acc.assign((size_t)ACC_FIELDS * cap, POISON_ACC);
    t.stamps.assign(2 * cap, POISON_I32);
    t.pierced.assign(has_pierced ? cap : 0, POISON_I32);
    return t;
}

static void assert_poison(const Map &t, int64_t from)
{
    for (int64_t d = from; d < t.cap; ++d) {
        assert(t.keys[d] == POISON_KEY && t.stamps[d] == POISON_I32 && t.stamps[t.cap + d] == POISON_I32);
        for (int c = 0; c < ACC_FIELDS; ++c) assert(t.acc[(size_t)c * t.cap + d] == POISON_ACC);
        if (t.has_pierced) assert(t.pierced[d] == POISON_I32);
    }
}

static void write_map(FILE *o, const Map &t, int64_t rows)
{
    std::vector<int64_t> k64(rows), a64((size_t)ACC_FIELDS * rows);
    std::vector<int32_t> s32(2 * rows), p32(t.has_pierced ? rows : 0);
    for (int64_t d = 0; d < rows; ++d) {
        assert(d == 0 || t.keys[d - 1] < t.keys[d]);
        k64[d] = (int64_t)t.keys[d];
        for (int c = 0; c < ACC_FIELDS; ++c) a64[(size_t)c * rows + d] = t.acc[(size_t)c * t.cap + d];
        s32[d] = t.stamps[d];
        s32[rows + d] = t.stamps[t.cap + d];
        if (t.has_pierced) p32[d] = t.pierced[d];
    }
    wr(o, k64); wr(o, a64); wr(o, s32); wr(o, p32);
}

// out[0..n] = exclusive scan of flag, out[n] = total
static std::vector<int> scan(const std::vector<int> &flag)
{
    std::vector<int> out(flag.size() + 1, 0);
    for (size_t i = 0; i < flag.size(); ++i) out[i + 1] = out[i] + flag[i];
    return out;
}

static void run_merge(FILE *f, FILE *o)
{
    const std::vector<int64_t> h = rd<int64_t>(f, 9);
    const int64_t ma = h[0], mb = h[3], ocap = h[6], add_dropped = h[8];
    const bool same = h[7] != 0;
    const Map A = read_map(f, ma, h[1], h[2] != 0);
    const Map B = same ? A : read_map(f, mb, h[4], h[5] != 0);
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
        for (int64_t d = 0; d < ocap; ++d) assert(written[d] == (d < total ? 1 : 0));
        rows = total;
    }
    assert_poison(out, rows);
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
    const Map A = read_map(f, m, h[1], h[2] != 0);
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
    assert_poison(out, runs);
    wr(o, counters); wr(o, state);
    write_map(o, out, runs);
}

int main(int argc, char **argv)
{
    assert(argc == 3);
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    assert(f && o);
    const int64_t mode = rd<int64_t>(f, 1)[0];
    assert(mode == 0 || mode == 1);
    if (mode == 0) run_merge(f, o); else run_regrid(f, o);
    fclose(o);
    fclose(f);
    return 0;
}
