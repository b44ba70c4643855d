"""Time the accumulated scene cloud (include/pcacc.h C4, pcaccumulation_amd/accumulate.py) on a scene's worth of windows and, beside it on the
same machine and inputs, what a user does without it: the copy of every window to the host plus the numpy restatement of the same contract
(tests/accumulate_reference.py: np.unique over the keys, int64 sums, a dict for the map).
  scene   --windows 40 windows of 5 x 160 k synthetic LiDAR-scan points (synthetic.make_sequence(mode='lidar_scan')), a pose that drifts 2 m and
          0.5 degrees per window, one map at --voxel 0.1 m starting from --capacity rows (the growth is part of the time)
GPU legs: device events around each add (kernels, the state read-back and any re-allocation included) and around extract; the median add of every
quarter of the scene is reported, as the map grows.  The two maps are compared at the end (equality).  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate.py [--windows 40] [--no-baseline] [--out profiles/accum_bench.txt]"""
import time

import numpy as np

from accum_bench import Report, header, parser, scene, timed


def parse_args(argv=None):
    return parser('accum_bench.txt', capacity=True).parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--capacity %d' % a.capacity, 'GPU: device events around each call; host: perf_counter')).emit
    windows = [(pts, mv, T) for _, pts, mv, T in scene(a, dev)]
    warm = AccumulatedCloud(a.voxel, dev, a.capacity)                         # warm-up: code objects, allocator
    warm.add(windows[0][0], windows[0][2], windows[0][1], 0).extract()
    del warm
    torch.cuda.synchronize()
    m = AccumulatedCloud(a.voxel, dev, a.capacity)
    times, sizes = [], []
    for k, (pts, mv, T) in enumerate(windows):
        times.append(timed(lambda: m.add(pts, T, mv, k))[0])
        sizes.append(m.num_voxels)
    t_extract, cloud = timed(lambda: m.extract(min_count=2, max_moving_fraction=0.0))
    n_pts = sum(w[0].shape[0] for w in windows)
    emit('GPU: %d windows, %d points -> %d voxels (capacity %d at the end, %d dropped); add median %.2f ms, total %.1f ms; '
         'extract(min_count=2, max_moving_fraction=0.0) %.2f ms -> %d voxels'
         % (a.windows, n_pts, m.num_voxels, m.capacity, m.dropped, float(np.median(times)), float(np.sum(times)), t_extract, cloud['count'].shape[0]))
    q = max(1, a.windows // 4)
    for lo in range(0, a.windows, q):
        hi = min(a.windows, lo + q)
        emit('  adds %2d-%2d: map %8d -> %8d voxels, median %.2f ms (%s)'
             % (lo, hi - 1, sizes[lo - 1] if lo else 0, sizes[hi - 1], float(np.median(times[lo:hi])), ' '.join('%.2f' % t for t in times[lo:hi])))
    if not a.no_baseline:
        import accumulate_reference as ref
        r = ref.ReferenceMap(a.voxel)
        host = []
        for k, (pts, mv, T) in enumerate(windows):
            t0 = time.perf_counter()
            r.add(pts.cpu().numpy(), T, mv.cpu().numpy(), k)                  # the round trip a user makes today, then the same arithmetic in numpy
            host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = r.extract(min_count=2, max_moving_fraction=0.0)
        host_extract = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(x, y) for x, y in zip(m.records(), r.records())) and \
            all(cloud[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in want)
        emit('host: copy to the host + numpy restatement: add median %.0f ms, total %.0f ms; extract %.0f ms; maps and extracts identical: %s'
             % (float(np.median(host)), float(np.sum(host)), host_extract, same))


if __name__ == '__main__':
    main()
