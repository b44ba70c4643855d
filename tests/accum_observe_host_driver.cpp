// Host build of pcaccumulation_amd/csrc/accum_observe.h (tests/test_accumulate_observe.py): ONE pcacc_accum_observe call and ONE lookup on the table it
// leaves, stage by stage as accum_observe.hip runs them -- count, offsets, emit, sort, runs, search, decide, merge, lookup -- on the CPU with every index
// assert-checked (-DPCACC_HOST_CHECK), before anything runs on a GPU.
// The input table stands at its capacity with misleading rows behind row m; the emitted keys and the output table are poisoned first: every destination
// is written exactly once, keys ascend, and what lies behind visit V (until the padding) and behind the last row is asserted untouched.
// Every walked ray is walked by accp_ray (accum_pierce.h) too, against a table of its own visits: the two visit sequences are asserted equal.
//   in : i64 n, S, m, in_capacity, out_capacity, visit_capacity, stamp, max_steps, has_moving, has_index, has_pose, use_range, n_lookup, lookup_coords,
//        min_rays, has_lookup_pose; f64 voxel_size, margin, max_range; f32 points[n][3]; u8 moving[n]; f64 origins[S][3]; i32 origin_index[n]; f64 pose[16];
//        i64 keys[m]; i64 rays[m]; i32 stamps[2][m]; i64 state[16]; f32 lookup_points[n_lookup][3] or i32 lookup_coords[n_lookup][3]; f64 lookup_pose[16]
//   out: i64 state[16]; i64 call_counters[5]; i64 rows; i64 keys[rows]; i64 rays[rows]; i32 stamps[2][rows] (the output table after OK, the input table
//        otherwise); u8 status[n_lookup]; i64 rays[n_lookup]; i32 stamps[2][n_lookup]; i64 counters[4]
#include <algorithm>

#include "accum_observe.h"
#include "accum_host.h"

enum { NUM_VOXELS = 0, STATUS = 1, NEEDED = 2, NEEDED_VISITS = 3, CALL_VISITS = 4, CALL_VOXELS = 5, WALKED = 6 };      // include/pcacc.h PCACC_OBSERVE_*

struct Seq {                                                                     // accp_ray's hit: the positions in visiting order
    std::vector<int64_t> *at;
    int64_t m;
    void operator()(int64_t pos) const { PCACC_BOUND(pos, m); at->push_back(pos); }
};

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 16);
    const std::vector<double> g = rd<double>(f, 3);
    const int64_t n = h[0], S = h[1], m_in = h[2], in_cap = h[3], out_cap = h[4], C = h[5], n_look = h[12], min_rays = h[14];
    const int32_t stamp = (int32_t)h[6];
    const int max_steps = (int)h[7];
    const bool use_range = h[11] != 0;
    const double voxel_size = g[0], margin = g[1], max_range = g[2];
    assert(n >= 0 && S >= 1 && m_in >= 0 && in_cap >= m_in && out_cap >= 1 && C >= 1 && max_steps >= 1 && max_steps <= ACCP_MAX_STEPS);
    assert(voxel_size > 0.0 && margin >= 0.0 && acco_visits_fit(n, max_steps) && n_look >= 0);
    const std::vector<float> points = rd<float>(f, 3 * n);
    const std::vector<uint8_t> moving = rd<uint8_t>(f, n);
    const std::vector<double> origins = rd<double>(f, 3 * S);
    const std::vector<int32_t> index = rd<int32_t>(f, n);
    const std::vector<double> pose = rd<double>(f, 16);
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = h[10] ? pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    // the input table at its capacity; rows past m: a key that would mislead any search that read it, a ray count and stamps no result may show
    std::vector<u64> in_keys(std::max<int64_t>(in_cap, 1), 0);
    std::vector<int64_t> in_rays(std::max<int64_t>(in_cap, 1), 77);
    std::vector<int32_t> in_stamps(2 * std::max<int64_t>(in_cap, 1), -7);
    {
        const std::vector<int64_t> k = rd<int64_t>(f, m_in), r = rd<int64_t>(f, m_in);
        const std::vector<int32_t> s = rd<int32_t>(f, 2 * m_in);
        for (int64_t i = 0; i < m_in; ++i) {
            in_keys[i] = (u64)k[i]; in_rays[i] = r[i]; in_stamps[i] = s[i]; in_stamps[in_cap + i] = s[m_in + i];
            assert(i == 0 || in_keys[i - 1] < in_keys[i]);
        }
    }
    std::vector<int64_t> state = rd<int64_t>(f, 16);

    // K0 begin
    const bool bad = state[NUM_VOXELS] < 0 || state[NUM_VOXELS] > in_cap;
    const int64_t m = bad ? 0 : state[NUM_VOXELS];
    assert(bad || m == m_in);

    // K1 count, and the walk of C7 beside it
    std::vector<int> count(n, 0);
    std::vector<int64_t> call(5, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t row = accp_origin_index(h[9] ? (int64_t)index[i] : 0, S);
        if (row >= 0) PCACC_BOUND(row, S);
        const double none[3] = {0.0, 0.0, 0.0};
        const double *origin = row >= 0 ? origins.data() + 3 * row : none;
        const bool mv = h[8] && moving[i];
        AccoCount counting;
        const AccoWalk r = acco_walk(T, points.data() + 3 * i, origin, row >= 0, mv, voxel_size, margin, use_range, max_range, max_steps, counting);
        assert(r.status == ACCP_WALKED || r.status == ACCP_DROPPED || r.status == ACCP_SKIPPED);
        assert(r.visits >= 0 && r.visits <= max_steps && (!r.truncated || r.visits == max_steps));
        assert(r.status == ACCP_WALKED ? r.visits >= 1 : (r.visits == 0 && !r.truncated));
        count[i] = r.visits;
        call[r.status] += 1; call[3] += r.truncated; call[4] += r.visits;
        // the same ray through accp_ray against the sorted list of its own visits: every visit hits, in the same order
        std::vector<u64> own(r.visits, POISON_KEY);
        AccoEmit own_emit = {own.data(), 0, r.visits};
        const AccoWalk again = acco_walk(T, points.data() + 3 * i, origin, row >= 0, mv, voxel_size, margin, use_range, max_range, max_steps, own_emit);
        assert(again.status == r.status && again.visits == r.visits && again.truncated == r.truncated && own_emit.at == r.visits);
        std::vector<u64> sorted_own(own);
        std::sort(sorted_own.begin(), sorted_own.end());
        for (size_t k = 1; k < sorted_own.size(); ++k) assert(sorted_own[k - 1] < sorted_own[k]);      // monotone walk: no voxel twice
        sorted_own.push_back(ACC_INVALID_KEY);                                   // never empty; not a row (m = visits)
        std::vector<int32_t> no_stamps(2 * sorted_own.size(), 0);
        std::vector<int64_t> seq;
        Seq hit = {&seq, r.visits};
        const AccpRay c7 = accp_ray(T, points.data() + 3 * i, origin, row >= 0, mv, voxel_size, margin, use_range, max_range, false, 0, max_steps,
                                    sorted_own.data(), no_stamps.data(), (int64_t)sorted_own.size(), (int64_t)r.visits, hit);
        assert(c7.status == r.status && c7.truncated == r.truncated && c7.visits == r.visits && c7.hits == r.visits && (int64_t)seq.size() == r.visits);
        for (int64_t k = 0; k < r.visits; ++k) assert(sorted_own[seq[k]] == own[k]);
    }
    assert(call[0] + call[1] + call[2] == n);

    // offsets
    const std::vector<int> offsets = scan(count);
    const int64_t V_all = offsets[n];
    assert(V_all == call[4]);

    // K2 decide
    const int visits_status = acco_decide_visits(bad, V_all, C);
    state[CALL_VISITS] = V_all;
    const bool emit = visits_status == ACCO_OK;
    const int64_t V = emit ? V_all : 0;
    if (!emit) {
        state[STATUS] = visits_status;
        if (visits_status == ACCO_TOO_MANY) state[NEEDED_VISITS] = V_all;
    }

    // K3 emit: poison first, every slot below V written exactly once, nothing behind V; then the padding up to C
    const int64_t spare = 3;
    std::vector<u64> key_a(C + spare, POISON_KEY);
    if (emit) {
        int64_t expect = 0;
        for (int64_t i = 0; i < n; ++i) {
            AccoEmit visit = {key_a.data(), 0, 0};
            assert(acco_slots(offsets.data(), i, n, V, &visit.at, &visit.end));
            assert(visit.at == expect && visit.end <= V && visit.end <= C);       // the slots tile [0, V) in ray order
            expect = visit.end;
            if (visit.at == visit.end) continue;
            const int64_t row = accp_origin_index(h[9] ? (int64_t)index[i] : 0, S);
            const double none[3] = {0.0, 0.0, 0.0};
            const double *origin = row >= 0 ? origins.data() + 3 * row : none;
            acco_walk(T, points.data() + 3 * i, origin, row >= 0, h[8] && moving[i], voxel_size, margin, use_range, max_range, max_steps, visit);
            assert(visit.at == visit.end);                                       // the ray wrote exactly its count
        }
        assert(expect == V);
        for (int64_t i = 0; i < V; ++i) assert(key_a[i] != POISON_KEY && key_a[i] != ACC_INVALID_KEY);
    }
    for (int64_t i = V; i < C + spare; ++i) assert(key_a[i] == POISON_KEY);
    for (int64_t i = V; i < C; ++i) key_a[i] = ACC_INVALID_KEY;

    // sort
    std::vector<u64> key_b(key_a.begin(), key_a.begin() + C);
    std::sort(key_b.begin(), key_b.end());

    // K4 heads + scan
    std::vector<int> head(C);
    for (int64_t i = 0; i < C; ++i) head[i] = acco_head(key_b.data(), i, V);
    const std::vector<int> vox = scan(head);
    const int64_t R = vox[C];
    assert(R >= 0 && R <= V);

    // K5 runs
    std::vector<u64> run_key(C, POISON_KEY);
    std::vector<int> run_start(C + 1, -1);
    run_start[R] = (int)V;
    for (int64_t i = 0; i < V; ++i) {
        if (!head[i]) continue;
        const int64_t r = accum_run_index(vox[i], 1, R);
        assert(r >= 0);
        PCACC_BOUND(r, R);
        assert(run_start[r] == -1);
        run_key[r] = key_b[i];
        run_start[r] = (int)i;
    }
    int64_t length_sum = 0;
    for (int64_t r = 0; r < R; ++r) {
        assert(r == 0 || run_key[r - 1] < run_key[r]);
        assert(acco_run_length(run_start.data(), r, R) >= 1);
        length_sum += acco_run_length(run_start.data(), r, R);
    }
    assert(length_sum == V);

    // K6 search + scan
    std::vector<int> miss(C, 0), pos(C, 0);
    for (int64_t j = 0; j < R; ++j) pos[j] = (int)acco_search(in_keys.data(), m, run_key[j], &miss[j]);
    const std::vector<int> mrank = scan(miss);

    // K7 decide
    bool go = false;
    int64_t total = 0;
    if (emit) {
        total = m + mrank[C];
        state[NEEDED] = total;
        state[CALL_VOXELS] = R;
        state[STATUS] = acco_decide_rows(total, out_cap);
        go = state[STATUS] == ACCO_OK;
        if (go) {
            state[NUM_VOXELS] = total;
            for (int k = 0; k < 5; ++k) state[WALKED + k] += call[k];
        }
    }

    // K8 merge into a poisoned table
    std::vector<u64> out_keys(out_cap, POISON_KEY);
    std::vector<int64_t> out_rays(out_cap, POISON_ACC);
    std::vector<int32_t> out_stamps(2 * out_cap, POISON_I32);
    if (go) {
        std::vector<int> written(out_cap, 0);
        for (int64_t p = 0; p < m; ++p) {
            const int64_t d = acco_merge_old(p, in_keys.data(), in_rays.data(), in_stamps.data(), in_cap, m, run_key.data(), run_start.data(), R, mrank.data(), total,
                                             stamp, out_keys.data(), out_rays.data(), out_stamps.data(), out_cap);
            assert(d >= 0 && d < total);
            ++written[d];
        }
        for (int64_t j = 0; j < R; ++j) {
            const int64_t d = acco_merge_new(j, run_key.data(), run_start.data(), R, miss.data(), pos.data(), mrank.data(), total, stamp, out_keys.data(),
                                             out_rays.data(), out_stamps.data(), out_cap);
            assert(miss[j] ? (d >= 0 && d < total) : d == -1);
            if (d >= 0) ++written[d];
        }
        assert_written_once(written, total);
        for (int64_t d = 1; d < total; ++d) assert(out_keys[d - 1] < out_keys[d]);
    }
    for (int64_t d = go ? total : 0; d < out_cap; ++d)
        assert(out_keys[d] == POISON_KEY && out_rays[d] == POISON_ACC && out_stamps[d] == POISON_I32 && out_stamps[out_cap + d] == POISON_I32);

    // the table the call leaves
    const u64 *keys = go ? out_keys.data() : in_keys.data();
    const int64_t *rays = go ? out_rays.data() : in_rays.data();
    const int32_t *stamps = go ? out_stamps.data() : in_stamps.data();
    const int64_t cap = go ? out_cap : in_cap, rows = go ? total : m_in;
    wr(o, state);
    wr(o, call);
    wr1(o, rows);
    std::vector<int64_t> k64(rows), r64(rows);
    std::vector<int32_t> s32(2 * rows);
    for (int64_t d = 0; d < rows; ++d) { k64[d] = (int64_t)keys[d]; r64[d] = rays[d]; s32[d] = stamps[d]; s32[rows + d] = stamps[cap + d]; }
    wr(o, k64); wr(o, r64); wr(o, s32);

    // lookup: every output poisoned first, every row written
    const std::vector<float> look_p = rd<float>(f, h[13] ? 0 : 3 * n_look);
    const std::vector<int32_t> look_c = rd<int32_t>(f, h[13] ? 3 * n_look : 0);
    const std::vector<double> look_pose = rd<double>(f, 16);
    double LT[12];
    for (int k = 0; k < 12; ++k) LT[k] = h[15] ? look_pose[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    std::vector<uint8_t> l_status = poisoned<uint8_t>(n_look);
    std::vector<int64_t> l_rays = poisoned<int64_t>(n_look), l_counters(4, 0);
    std::vector<int32_t> l_stamps = poisoned<int32_t>(2 * n_look);
    for (int64_t i = 0; i < n_look; ++i) {
        u64 key = 0;
        int64_t q[3];
        const bool valid = h[13] ? acco_coord_key(look_c.data() + 3 * i, &key) : accum_point(LT, look_p.data() + 3 * i, voxel_size, &key, q);
        int64_t r;
        int32_t t0, t1;
        const int status = acco_lookup(valid, key, keys, rays, stamps, cap, rows, min_rays, &r, &t0, &t1);
        assert((status & ~7) == 0 && (!(status & ACCO_ENOUGH) || (status & ACCO_SEEN)) && (!(status & ACCO_SEEN) || (status & ACCO_VALID)));
        assert((status & ACCO_SEEN) || (r == 0 && t0 == 0 && t1 == 0));
        l_status[i] = (uint8_t)status; l_rays[i] = r; l_stamps[i] = t0; l_stamps[n_look + i] = t1;
        l_counters[0] += 1; l_counters[1] += (status & ACCO_VALID) != 0; l_counters[2] += (status & ACCO_SEEN) != 0; l_counters[3] += (status & ACCO_ENOUGH) != 0;
    }
    wr(o, l_status); wr(o, l_rays); wr(o, l_stamps); wr(o, l_counters);
    close_io(f, o);
    return 0;
}
