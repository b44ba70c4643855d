// Host build of the ICP refinement (pcaccumulation_amd/csrc/icp_grid.h, icp_round.h): the cell / key arithmetic, the hash probe, the 27-cell walk, the
// slice sums in the kernels' order and the whole round logic the kernels of icp.hip run, compiled with g++ and PCACC_HOST_CHECK so that EVERY table
// index is assert-checked.  tests/test_icp.py builds it, feeds it a scene (far-away, NaN and Inf points included), compares the correspondences with
// brute force and the loop's results with the numpy restatement -- before anything runs on a GPU; the GPU test then holds the kernels to this build
// bit for bit.
//   usage: icp_host_driver <scene.bin> <out.bin> [<max_iter> <loop.bin>]
//   scene: int64 n, n_seg, n_jobs; double threshold; float points[n][3]; int32 offsets[n_seg + 1]; int32 jobs[n_jobs][2]; double init[n_jobs][16]
//   out:   per job, per source point (segment order): int64 index of its correspondence in `points` under the initial pose, or -1
//   loop:  per job: double pose[16], fitness, rmse; int32 iterations, status -- the loop stops where the device's stops: the rounds after `done`
//          would return at once
#ifndef PCACC_HOST_CHECK
#define PCACC_HOST_CHECK
#endif
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "icp_round.h"

template <class T>
static void read_n(FILE *f, T *p, size_t count)
{
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "scene file too short\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 5) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    double thr;
    read_n(f, head, 3);
    read_n(f, &thr, 1);
    const int64_t n = head[0], n_seg = head[1], n_jobs = head[2];
    std::vector<float> points(3 * n);
    std::vector<int32_t> offsets(n_seg + 1), jobs(2 * n_jobs);
    std::vector<double> init(16 * n_jobs);
    read_n(f, points.data(), points.size());
    read_n(f, offsets.data(), offsets.size());
    read_n(f, jobs.data(), jobs.size());
    read_n(f, init.data(), init.size());
    fclose(f);

    // the tables as icp_setup validates them
    for (int64_t s = 0; s <= n_seg; ++s) assert(offsets[s] >= 0 && offsets[s] <= n && (s == n_seg || offsets[s] <= offsets[s + 1]));
    std::vector<int32_t> tflag(n_seg, 0);
    for (int64_t j = 0; j < n_jobs; ++j) {
        assert(jobs[2 * j] >= 0 && jobs[2 * j] < n_seg && jobs[2 * j + 1] >= 0 && jobs[2 * j + 1] < n_seg);
        tflag[jobs[2 * j + 1]] = 1;
    }

    // icp_insert / scan / icp_fill, sequentially (the fill runs BACKWARDS: the walk must not depend on the order inside a cell's list)
    uint32_t slots = 64;
    while ((int64_t)slots < 2 * n) slots <<= 1;
    const uint32_t mask = slots - 1;
    std::vector<unsigned long long> keys(slots, 0);
    std::vector<int32_t> cnt(slots, 0), start(slots + 1, 0), pslot(n, -1), list(n > 0 ? n : 1, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int seg = icp_segment_of(offsets.data(), (int)n_seg, i);
        if (seg < 0) continue;
        PCACC_BOUND(seg, n_seg);
        if (!tflag[seg]) continue;
        const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        int c[3];
        if (!icp_target_cell(p, thr, c)) continue;
        for (int a = 0; a < 3; ++a) assert(c[a] >= ICP_CELL_MIN && c[a] <= ICP_CELL_MAX);
        const unsigned long long key = icp_key(seg, c[0], c[1], c[2]);
        assert(key != 0 && (key >> 48) == (unsigned long long)(seg + 1));
        uint32_t s = icp_hash(key, mask);
        uint32_t probes = 0;
        for (; probes <= mask; ++probes, s = (s + 1) & mask) {
            PCACC_BOUND(s, slots);
            if (keys[s] == 0) keys[s] = key;
            if (keys[s] == key) break;
        }
        assert(probes <= mask);
        cnt[s]++;
        pslot[i] = (int32_t)s;
    }
    for (uint32_t s = 0; s < slots; ++s) start[s + 1] = start[s] + cnt[s];
    assert(start[slots] <= n);
    std::vector<int32_t> cursor(slots, 0);
    for (int64_t i = n - 1; i >= 0; --i) {
        const int32_t s = pslot[i];
        if (s < 0) continue;
        const int64_t e = (int64_t)start[s] + cursor[s]++;
        PCACC_BOUND(e, start[s + 1]);
        PCACC_BOUND(e, n);
        list[e] = (int32_t)i;
    }

    IcpGrid g;
    g.keys = keys.data(); g.start = start.data(); g.list = list.data(); g.points = points.data();
    g.mask = mask; g.n = n; g.n_list = start[slots]; g.h = thr;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int64_t j = 0; j < n_jobs; ++j) {
        const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
        for (int64_t i = offsets[src]; i < offsets[src + 1]; ++i) {
            PCACC_BOUND(i, n);
            double q[3], d2 = 0.0;
            icp_apply(&init[16 * j], &points[3 * i], q);
            const int64_t m = icp_nearest(g, tgt, q, thr * thr, &d2);
            if (m >= 0) {
                assert(m >= offsets[tgt] && m < offsets[tgt + 1]);     // a correspondence never leaves the job's target segment
                assert(d2 <= thr * thr);
            }
            fwrite(&m, sizeof(m), 1, o);
        }
    }
    fclose(o);
    if (argc != 5) return 0;

    const int max_iter = atoi(argv[3]);
    const int slices = icp_slices(n, (int32_t)n_jobs);
    o = fopen(argv[4], "wb");
    if (!o) return 2;
    for (int64_t j = 0; j < n_jobs; ++j) {
        const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
        IcpState st;
        pcacc_pose_seed(st.T, &init[16 * j]);
        st.fit = st.rmse = 0.0;
        st.done = st.iters = st.status = st.pad = 0;
        double pose[16], fit = 0.0, rmse = 0.0;
        int32_t iters = -1, status = -1;
        const IcpOut out = {pose, &fit, &rmse, &iters, &status};
        for (int round = 0; round <= max_iter && !st.done; ++round) {
            double sums[ICP_SUMS], part[ICP_SUMS];
            for (int k = 0; k < ICP_SUMS; ++k) sums[k] = 0.0;
            for (int s = 0; s < slices; ++s) {                        // icp_update: the slots in slice order
                int64_t a, b;
                icp_slice_bounds(offsets[src], offsets[src + 1], slices, s, &a, &b);
                assert(a >= offsets[src] && b <= offsets[src + 1]);
                icp_slice_sums(g, tgt, st.T, thr * thr, a, b, part);
                for (int k = 0; k < ICP_SUMS; ++k) sums[k] = sums[k] + part[k];
            }
            icp_round(&st, sums, (int64_t)offsets[src + 1] - offsets[src], (int64_t)offsets[tgt + 1] - offsets[tgt], round, max_iter, &out);
        }
        assert(st.done && iters >= 0 && iters <= max_iter);
        fwrite(pose, sizeof(double), 16, o);
        fwrite(&fit, sizeof(fit), 1, o);
        fwrite(&rmse, sizeof(rmse), 1, o);
        fwrite(&iters, sizeof(iters), 1, o);
        fwrite(&status, sizeof(status), 1, o);
    }
    fclose(o);
    return 0;
}
