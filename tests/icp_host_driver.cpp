// Host build of the ICP target index (pcaccumulation_amd/csrc/icp_grid.h): the cell / key arithmetic, the hash probe and the 27-cell walk the
// kernels of icp.hip run, compiled with g++ and ICP_HOST_CHECK so that EVERY table index is assert-checked.  tests/test_icp.py builds it, feeds
// it a scene (far-away, NaN and Inf points included) and compares the correspondences with brute force -- before anything runs on a GPU.
//   usage: icp_host_driver <scene.bin> <out.bin>
//   scene: int64 n, n_seg, n_jobs; double threshold; float points[n][3]; int32 offsets[n_seg + 1]; int32 jobs[n_jobs][2]; double init[n_jobs][16]
//   out:   per job, per source point (segment order): int64 index of its correspondence in `points`, or -1
#ifndef ICP_HOST_CHECK
#define ICP_HOST_CHECK
#endif
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "icp_grid.h"

template <class T>
static void read_n(FILE *f, T *p, size_t count)
{
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "scene file too short\n"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
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
        ICP_BOUND(seg, n_seg);
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
            ICP_BOUND(s, slots);
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
        ICP_BOUND(e, start[s + 1]);
        ICP_BOUND(e, n);
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
            ICP_BOUND(i, n);
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
    return 0;
}
