"""Time the merge and the regrid of accumulated scene clouds (include/pcacc.h C12, pcaccumulation_amd/accumulate.py) and, beside them on the same
machine and inputs, the yardstick the project already has -- the median add of the same session at the same map size -- and the path a user has
without them: records() of both maps to the host, a numpy join there, load().
  scene   tools/bench_accumulate.py's: --windows 40 windows of 5 x 160 k synthetic LiDAR-scan points, a pose that drifts 2 m and 0.5 degrees per window,
          --voxel 0.1 m.  Map A takes the first half of the windows, map B the second.
  legs    A.copy().merge(B); B.regrid(pose) at the same voxel size and at twice the voxel size; A.copy().merge(B, pose) -- device events around each call,
          read-backs and any re-allocation included, the copy() outside; the median of --repeats calls.
The merged map is compared with the host join (equality).  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_merge.py [--windows 40] [--repeats 5] [--no-baseline] [--out profiles/accum_merge_bench.txt]"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_accumulate import drift  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=40)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--pts-per-frame', type=int, default=160000)
    ap.add_argument('--voxel', type=float, default=0.1)
    ap.add_argument('--capacity', type=int, default=1 << 20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accum_merge_bench.txt'))
    a = ap.parse_args()
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    from pcaccumulation_amd.config import default_config
    from pcaccumulation_amd.synthetic import make_sequence
    dev = torch.device('cuda:0')
    cfg = default_config('waymo', 'test', n_sweeps=a.frames)
    lines = ['tools/bench_accumulate_merge.py --windows %d --frames %d --pts-per-frame %d --voxel %g --capacity %d --repeats %d   (%s; GPU: device events '
             'around each call; host: perf_counter)' % (a.windows, a.frames, a.pts_per_frame, a.voxel, a.capacity, a.repeats, torch.cuda.get_device_name(0))]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rng = np.random.RandomState(0)
    half = a.windows // 2
    maps, adds = [], []
    for lo, hi in ((0, half), (half, a.windows)):
        m, times = AccumulatedCloud(a.voxel, dev, a.capacity), []
        for k in range(lo, hi):
            s = make_sequence(500 + k, a.frames, a.pts_per_frame, cfg, mode='lidar_scan')
            pts = torch.from_numpy(np.ascontiguousarray(s['input_points'][:, :3], np.float32)).to(dev)
            mv = torch.from_numpy(rng.rand(pts.shape[0]) < 0.1).to(dev)
            if k == 0:                                                           # warm-up: code objects, allocator
                AccumulatedCloud(a.voxel, dev, a.capacity).add(pts, drift(k), mv, k).extract()
                torch.cuda.synchronize()
            times.append((timed(lambda: m.add(pts, drift(k), mv, k))[0], m.num_voxels))
        maps.append(m)
        adds.append(times)
    A, B = maps
    tail = [t for t, _ in adds[0][-max(1, half // 4):]]                          # the adds that met a map of about A's final size
    add_ms = float(np.median(tail))
    lines.append('maps: A = windows 0-%d, %d voxels (capacity %d); B = windows %d-%d, %d voxels; yardstick: median add of the last %d windows of A '
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
        lines.append('GPU: %-32s median %.2f ms = %.2f x the median add (%s) %s' % (name, float(np.median(times)), float(np.median(times)) / add_ms,
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
        lines.append('host: records() of both + numpy join + load(): median %.0f ms (%s); map identical to merge(B): %s'
                     % (float(np.median(host)), ' '.join('%.0f' % t for t in host), same))
        lines.append('host: a map under a pose or at another voxel size has no path without regrid: extract() + add() loses counts, flags, stamps and rays')
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
