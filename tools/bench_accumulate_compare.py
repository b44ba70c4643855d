"""Time the comparison of two accumulated scene clouds, the selection of half a map's rows and the difference of two maps (include/pcacc.h C13,
pcaccumulation_amd/accumulate.py) and, beside them on the same machine and inputs, the yardsticks the project already has: the median add of the same
session at the same map size, and the two routes a user has without them -- b.query(a.extract()['points']) plus the reverse on the device, and
records() of both maps to the host with a numpy searchsorted join there.
  scene   tools/bench_accumulate_merge.py's: --windows 40 windows of 5 x 160 k synthetic LiDAR-scan points, a pose that drifts 2 m and 0.5 degrees per
          window, --voxel 0.1 m.  Map A takes the first half of the windows, map B the second.
  legs    A.compare(B); A.select(every second row); A.difference(B) -- device events around each call, the counter read-back and every allocation
          included; the median of --repeats calls.
The host join's SAME / HELD counts are compared with compare's counters (equality).  Results go to --out.  Nothing is gated on them.
Usage: timeout -k 10 900 python tools/bench_accumulate_compare.py [--windows 40] [--repeats 5] [--no-baseline] [--out profiles/accum_compare_bench.txt]"""
import itertools
import time

import numpy as np

from accum_bench import Report, drift, header, parser, scene, timed


def host_join(a, b):
    """What a user does today: both maps' records to the host and a join of the sorted keys -> the keys both maps hold."""
    (ka, _, _), (kb, _, _) = a.records(), b.records()
    q = np.minimum(np.searchsorted(kb, ka), kb.shape[0] - 1)
    return int((kb[q] == ka).sum())


def parse_args(argv=None):
    return parser('accum_compare_bench.txt', capacity=True, repeats=5).parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--capacity %d --repeats %d' % (a.capacity, a.repeats),
                                'GPU: device events around each call; host: perf_counter')).emit

    def leg(name, call, what):
        times, out = [], None
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t, out = timed(call)
            times.append(t)
        emit('GPU: %-44s median %.2f ms = %.2f x the median add (%s) %s' % (name, float(np.median(times)), float(np.median(times)) / add_ms,
                                                                        ' '.join('%.2f' % t for t in times), what(out)))
        return out

    half = a.windows // 2
    windows = scene(a, dev)                                                      # one generator for both maps: B's windows follow A's
    maps, adds = [], []
    for n in (half, a.windows - half):
        m, times = AccumulatedCloud(a.voxel, dev, a.capacity), []
        for k, pts, mv, _ in itertools.islice(windows, n):
            if k == 0:                                                           # warm-up: code objects, allocator
                AccumulatedCloud(a.voxel, dev, a.capacity).add(pts, drift(k), mv, k).extract()
                torch.cuda.synchronize()
            times.append((timed(lambda: m.add(pts, drift(k), mv, k))[0], m.num_voxels))
        maps.append(m)
        adds.append(times)
    A, B = maps
    tail = [t for t, _ in adds[0][-max(1, half // 4):]]                          # the adds that met a map of about A's final size
    add_ms = float(np.median(tail))
    emit('maps: A = windows 0-%d, %d voxels (capacity %d); B = windows %d-%d, %d voxels; yardstick: median add of the last %d windows of A '
         '(map %d -> %d voxels, %d points each) %.2f ms' % (half - 1, A.num_voxels, A.capacity, half, a.windows - 1, B.num_voxels, len(tail),
                                                             adds[0][-len(tail) - 1][1] if len(adds[0]) > len(tail) else 0, A.num_voxels,
                                                             a.frames * a.pts_per_frame, add_ms))
    small = AccumulatedCloud(a.voxel, dev, 64).add(pts[:1000], None, None, 0)    # warm-up of the new code objects and of query's
    small.difference(small)
    small.query(small.extract()['points'])
    torch.cuda.synchronize()
    every_second = (torch.arange(A.num_voxels, device=dev) % 2) == 0
    counters = leg('A.compare(B)', lambda: A.compare(B), lambda out: '-> %r' % (out['counters'],))['counters']
    leg('A.select(every second row)', lambda: A.select(every_second), lambda out: '-> %d rows' % out.num_voxels)
    leg('A.difference(B)', lambda: A.difference(B), lambda out: '-> %d rows' % out.num_voxels)
    if not a.no_baseline:
        leg('B.query(A.extract()) + A.query(B.extract())', lambda: (B.query(A.extract()['points']), A.query(B.extract()['points'])),
            lambda out: '-> float32 centroids, one way each, no row of the other map\'s own voxel')
        host = []
        for _ in range(min(a.repeats, 3)):
            t0 = time.perf_counter()
            shared = host_join(A, B)
            host.append((time.perf_counter() - t0) * 1e3)
        same = all(counters[s][k] == shared for s in ('self', 'other') for k in ('same', 'held'))
        emit('host: records() of both + numpy searchsorted join: median %.0f ms (%s); %d keys in both maps; SAME and HELD of both sides equal it: %s'
             % (float(np.median(host)), ' '.join('%.0f' % t for t in host), shared, same))


if __name__ == '__main__':
    main()
