"""Time the merge and the regrid of accumulated scene clouds (include/pcacc.h C12, pcaccumulation_amd/accumulate.py) and, beside them on the same
machine and inputs, the yardstick the project already has -- the median add of the same session at the same map size -- and the path a user has
without them: records() of both maps to the host, a numpy join there, load().
  scene   tools/bench_accumulate.py's: --windows 40 windows of 5 x 160 k synthetic LiDAR-scan points, a pose that drifts 2 m and 0.5 degrees per window,
          --voxel 0.1 m.  Map A takes the first half of the windows, map B the second.
  legs    A.copy().merge(B); B.regrid(pose) at the same voxel size and at twice the voxel size; A.copy().merge(B, pose) -- device events around each call,
          read-backs and any re-allocation included, the copy() outside; the median of --repeats calls.
The merged map is compared with the host join (equality).  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_merge.py [--windows 40] [--repeats 5] [--no-baseline] [--out profiles/accum_merge_bench.txt]"""
import io
import itertools
import time

import numpy as np

from accum_bench import Report, drift, header, parser, scene, timed


def host_join(a, b, device):
    """What a user does today: both maps' records to the host, a numpy join, a load."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    (ka, aa, sa), (kb, ab, sb) = a.records(), b.records()
    keys, inv = np.unique(np.concatenate([ka, kb]), return_inverse=True)
    acc = np.zeros((keys.shape[0], 5), np.int64)
    np.add.at(acc, inv, np.concatenate([aa, ab], 1).T)
    first = np.full(keys.shape[0], np.iinfo(np.int32).max, np.int32)
    last = np.full(keys.shape[0], np.iinfo(np.int32).min, np.int32)
    np.minimum.at(first, inv, np.concatenate([sa[0], sb[0]]))
    np.maximum.at(last, inv, np.concatenate([sa[1], sb[1]]))
    buf = io.BytesIO()
    np.savez(buf, keys=keys, acc=np.ascontiguousarray(acc.T), stamps=np.stack([first, last]), voxel_size=np.float64(a.voxel_size),
             dropped=np.int64(a.dropped + b.dropped))
    buf.seek(0)
    return AccumulatedCloud.load(buf, device)


def parse_args(argv=None):
    return parser('accum_merge_bench.txt', capacity=True, repeats=5).parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--capacity %d --repeats %d' % (a.capacity, a.repeats),
                                'GPU: device events around each call; host: perf_counter')).emit
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
    pose = drift(3)
    AccumulatedCloud(a.voxel, dev, 64).merge(B.regrid(pose=pose))                # warm-up of the new code objects
    torch.cuda.synchronize()
    merged = None
    legs = (('merge(B)', lambda c: c.merge(B), True), ('B.regrid(pose)', lambda c: B.regrid(pose=pose), False),
            ('B.regrid(pose, voxel_size=%g)' % (2 * a.voxel), lambda c: B.regrid(pose=pose, voxel_size=2 * a.voxel), False),
            ('merge(B, pose)', lambda c: c.merge(B, pose=pose), True))
    for name, call, mutates in legs:
        times, out = [], None
        for _ in range(a.repeats):
            c = A.copy() if mutates else None
            torch.cuda.synchronize()
            t, out = timed(lambda: call(c))
            times.append(t)
            if name == 'merge(B)':
                merged = c
        what = ('-> %d rows, capacity %d' % (c.num_voxels, c.capacity)) if mutates else ('-> %d rows, %d dropped' % (out.num_voxels, out.dropped - B.dropped))
        emit('GPU: %-32s median %.2f ms = %.2f x the median add (%s) %s' % (name, float(np.median(times)), float(np.median(times)) / add_ms,
                                                                        ' '.join('%.2f' % t for t in times), what))
    if not a.no_baseline:
        host = []
        for _ in range(min(a.repeats, 3)):
            t0 = time.perf_counter()
            joined = host_join(A, B, dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        same = joined.num_voxels == merged.num_voxels and joined.dropped == merged.dropped and all(
            np.array_equal(x, y) for x, y in zip(joined.records(), merged.records()))
        emit('host: records() of both + numpy join + load(): median %.0f ms (%s); map identical to merge(B): %s'
             % (float(np.median(host)), ' '.join('%.0f' % t for t in host), same))
        emit('host: a map under a pose or at another voxel size has no path without regrid: extract() + add() loses counts, flags, stamps and rays')


if __name__ == '__main__':
    main()
