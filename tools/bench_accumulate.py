"""Time the accumulated scene cloud (include/pcacc.h C4, pcaccumulation_amd/accumulate.py) on a scene's worth of windows and, beside it on the
same machine and inputs, what a user does without it: the copy of every window to the host plus the numpy restatement of the same contract
(tests/accumulate_reference.py: np.unique over the keys, int64 sums, a dict for the map).
  scene   --windows 40 windows of 5 x 160 k synthetic LiDAR-scan points (synthetic.make_sequence(mode='lidar_scan')), a pose that drifts 2 m and
          0.5 degrees per window, one map at --voxel 0.1 m starting from --capacity rows (the growth is part of the time)
GPU legs: device events around each add (kernels, the state read-back and any re-allocation included) and around extract; the median add of every
quarter of the scene is reported, as the map grows.  The two maps are compared at the end (equality).  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate.py [--windows 40] [--no-baseline] [--out profiles/accum_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def drift(k):
    a = np.deg2rad(0.5 * k)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[:3, 3] = (2.0 * k, 0.1 * k, 0.0)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=40)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--pts-per-frame', type=int, default=160000)
    ap.add_argument('--voxel', type=float, default=0.1)
    ap.add_argument('--capacity', type=int, default=1 << 20)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accum_bench.txt'))
    a = ap.parse_args()
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    from pcaccumulation_amd.config import default_config
    from pcaccumulation_amd.synthetic import make_sequence
    dev = torch.device('cuda:0')
    cfg = default_config('waymo', 'test', n_sweeps=a.frames)
    lines = ['tools/bench_accumulate.py --windows %d --frames %d --pts-per-frame %d --voxel %g --capacity %d   (%s; GPU: device events around each '
             'call; host: perf_counter)' % (a.windows, a.frames, a.pts_per_frame, a.voxel, a.capacity, torch.cuda.get_device_name(0))]
    rng = np.random.RandomState(0)
    windows = []
    for k in range(a.windows):
        s = make_sequence(500 + k, a.frames, a.pts_per_frame, cfg, mode='lidar_scan')
        pts = np.ascontiguousarray(s['input_points'][:, :3], np.float32)
        windows.append((torch.from_numpy(pts).to(dev), torch.from_numpy(rng.rand(pts.shape[0]) < 0.1).to(dev), drift(k)))
    warm = AccumulatedCloud(a.voxel, dev, a.capacity)                         # warm-up: code objects, allocator
    warm.add(windows[0][0], windows[0][2], windows[0][1], 0).extract()
    del warm
    torch.cuda.synchronize()
    m = AccumulatedCloud(a.voxel, dev, a.capacity)
    times, sizes = [], []
    for k, (pts, mv, T) in enumerate(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.add(pts, T, mv, k)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        sizes.append(m.num_voxels)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cloud = m.extract(min_count=2, max_moving_fraction=0.0)
    e1.record()
    torch.cuda.synchronize()
    t_extract = e0.elapsed_time(e1)
    n_pts = sum(w[0].shape[0] for w in windows)
    lines.append('GPU: %d windows, %d points -> %d voxels (capacity %d at the end, %d dropped); add median %.2f ms, total %.1f ms; '
                 'extract(min_count=2, max_moving_fraction=0.0) %.2f ms -> %d voxels'
                 % (a.windows, n_pts, m.num_voxels, m.capacity, m.dropped, float(np.median(times)), float(np.sum(times)), t_extract, cloud['count'].shape[0]))
    q = max(1, a.windows // 4)
    for lo in range(0, a.windows, q):
        hi = min(a.windows, lo + q)
        lines.append('  adds %2d-%2d: map %8d -> %8d voxels, median %.2f ms (%s)'
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
        lines.append('host: copy to the host + numpy restatement: add median %.0f ms, total %.0f ms; extract %.0f ms; maps and extracts identical: %s'
                     % (float(np.median(host)), float(np.sum(host)), host_extract, same))
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
