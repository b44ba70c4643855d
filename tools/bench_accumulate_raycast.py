"""Time the ray cast of the accumulated scene cloud (include/pcacc.h C10, AccumulatedCloud.raycast / render_range_image) on the 40-window drifting
scene of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m, the sensor 1.8 m above the window's origin) and, beside it on the same machine
and inputs, what a user does without it: the copy of the keys to the host and a ray cast there.
  (i)    the last window's 800 000 points as targets against the map of all windows: to the target (max_range=None, margin = 2 voxels) and at
         --max-range, each with and without min_count=2, max_moving_fraction=0.0, and each at min_range 0 and --min-range (the cloud of this scene
         fills the sensor's own voxel, so at min_range 0 a ray hits where it starts; a sensor's blind zone skips that); beside them one see_through call on the same rays in the same
         run -- a distance, not a target: a ray that stops at its first hit visits fewer voxels.  How many fewer is reported from the counters:
         visits per ray of each call, and of the walk that nothing stops (a filter that keeps no voxel).
  (ii)   render_range_image at 64 x 2048 from the last pose, max_range 30 and 80, min_range 0 and --min-range, on the full map and on the map pruned to a --box metre box.
  (iii)  a host baseline on a --sample sub-sample of (i)'s rays: the walk of tests/accumulate_raycast_reference.py in plain Python with the rows by
         np.searchsorted in the copied keys; its hit count must equal the kernel's on the same rays.
Device events around each call, one warm-up, median of --repeat.  Run it under a time limit of its own (timeout -k 10 600 python tools/...).
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
figures give sizes and memory behaviour, not what a street looks like.  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_raycast.py [--windows 40] [--max-range 30] [--min-range 2] [--box 50] [--sample 2000] [--repeat 5] [--no-baseline]
       [--out profiles/accum_raycast_bench.txt]"""
import time

import numpy as np

from accum_bench import BIAS, SENSOR, Report, drift, header, parser, scene, timed_repeat

NAMES = ('rays', 'dropped', 'skipped', 'hit', 'missed', 'truncated', 'visits')


class SortedKeys(object):
    """The `kept` of accumulate_raycast_reference.ray on the copied records: a voxel is found by np.searchsorted in the keys, no filter."""

    def __init__(self, records):
        self.keys, self.acc, _ = records

    def get(self, c):
        k = ((c[0] + BIAS) << 42) | ((c[1] + BIAS) << 21) | (c[2] + BIAS)
        p = int(np.searchsorted(self.keys, k))
        if p >= self.keys.shape[0] or int(self.keys[p]) != k:
            return None
        n = float(self.acc[0, p])
        return p, [(float(self.acc[2 + a, p]) / n) * (1.0 / 65536.0) for a in range(3)]


def parse_args(argv=None):
    ap = parser('accum_raycast_bench.txt', repeat=5)
    ap.add_argument('--max-range', type=float, default=30.0)
    ap.add_argument('--min-range', type=float, default=2.0)
    ap.add_argument('--box', type=float, default=50.0)
    ap.add_argument('--sample', type=int, default=2000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--max-range %g --min-range %g --box %g --repeat %d' % (a.max_range, a.min_range, a.box, a.repeat),
                                'GPU: device events around each call, one warm-up, median of %d; host: perf_counter' % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    scan = None
    for k, scan, mv, T in scene(a, dev):
        m.add(scan, T, mv, k)
        if k % 10 == 9:
            print('window %d: %d voxels' % (k, m.num_voxels), flush=True)
    pose = drift(a.windows - 1)
    n = scan.shape[0]
    filt = dict(min_count=2, max_moving_fraction=0.0)
    margin = 2.0 * a.voxel

    def report(what, res, ms):
        c = res['counters'].tolist() if hasattr(res, 'keys') else None
        tail = '' if c is None else '; ' + ', '.join('%s %d' % kv for kv in zip(NAMES, c)) + ' (%.1f visits per walked ray)' % (c[6] / max(c[3] + c[4] + c[5], 1))
        emit('  GPU %s: median %.3f ms, min %.3f, max %.3f%s' % (what, float(np.median(ms)), min(ms), max(ms), tail))

    # (i) the last window's points as targets
    emit('(i) the full map: %d voxels; the last window\'s %d points as targets, the sensor at %s under the last pose' % (m.num_voxels, n, SENSOR[0].tolist()))
    legs = []
    for near in (0.0, a.min_range):                                              # this cloud fills the sensor's own voxel: at min_range 0 a ray hits where it starts
        for tag, f in (('no filter', dict()), ('min_count=2, max_moving_fraction=0.0', filt)):
            legs.append(('raycast to the target, margin %g, min_range %g, %s' % (margin, near, tag), dict(margin=margin, min_range=near, **f)))
            legs.append(('raycast, max_range %g, min_range %g, %s' % (a.max_range, near, tag), dict(max_range=a.max_range, min_range=near, **f)))
    legs.append(('raycast to the target, margin %g, a filter that keeps nothing (the walk that nothing stops: see_through\'s visits)' % margin,
                 dict(margin=margin, min_count=1 << 40)))
    for what, args in legs:
        report(what, *timed_repeat(lambda: m.raycast(scan, SENSOR, pose=pose, **args), a.repeat))
    _, ms = timed_repeat(lambda: m.see_through(scan, SENSOR, pose=pose, margin=margin), a.repeat)
    c = m._pierce_counters.tolist()
    emit('  GPU see_through of the same rays, margin %g, no stamp (beside it, a distance and not a target: it never stops and adds to a sidecar): median '
         '%.3f ms, min %.3f, max %.3f; per call walked %d, hits %d' % (margin, float(np.median(ms)), min(ms), max(ms), c[0] // (a.repeat + 1), c[4] // (a.repeat + 1)))

    # (iii) the host baseline, on the full map
    if not a.no_baseline:
        import accumulate_raycast_reference as yref
        t0 = time.perf_counter()
        records = m.records()
        pts = scan.cpu().numpy()
        t_copy = time.perf_counter() - t0
        pick = np.random.RandomState(1).choice(n, min(a.sample, n), replace=False)
        pick.sort()
        lookup = SortedKeys(records)
        Tl = [[float(v) for v in row] for row in pose[:3]]
        t0 = time.perf_counter()
        status = [yref.ray(lookup, Tl, pts[i], SENSOR[0], a.voxel, a.min_range, a.max_range, 0.0, 4096) for i in pick]
        t_host = time.perf_counter() - t0
        hits = sum(r['status'] == yref.HIT for r in status)
        visits = sum(r['visits'] for r in status)
        sel = torch.from_numpy(pick).to(dev)
        res, ms = timed_repeat(lambda: m.raycast(scan[sel], SENSOR, pose=pose, max_range=a.max_range, min_range=a.min_range), a.repeat)
        got = res['counters'].tolist()
        emit('(iii) host, a sub-sample of %d rays of (i), max_range %g, min_range %g, no filter: copy of the records (%d voxels) and the scan %.2f s; the walk in plain Python '
             'with np.searchsorted %.2f s = %.2f ms per ray (%.0f s for the whole window at that rate); hits %d, visits %d; the kernel on the same rays: hits %d, '
             'visits %d (%s), median %.3f ms for the call'
             % (pick.shape[0], a.max_range, a.min_range, records[0].shape[0], t_copy, t_host, 1e3 * t_host / pick.shape[0], t_host / pick.shape[0] * n, hits, visits,
                got[native.RAYCAST_N_HIT], got[native.RAYCAST_N_VISITS], 'equal' if (hits, visits) == (got[3], got[6]) else 'DIFFERENT', float(np.median(ms))))
        assert hits == got[native.RAYCAST_N_HIT], (hits, got)
        del records, lookup

    # (ii) range images from the last pose
    sensor_pose = np.array(pose, np.float64)
    sensor_pose[:3, 3] = pose[:3, :3] @ SENSOR[0] + pose[:3, 3]

    def images(tag):
        emit('(ii) %s: %d voxels; render_range_image 64 x 2048, vertical field +3 .. -25 degrees, from the last pose' % (tag, m.num_voxels))
        for max_range in (30.0, 80.0):
            for near in (0.0, a.min_range):
                res, ms = timed_repeat(lambda: m.render_range_image(sensor_pose, 64, 2048, np.deg2rad(3.0), np.deg2rad(-25.0), max_range, min_range=near), a.repeat)
                report('max_range %g, min_range %g, no filter (the host-side directions and their copy are inside the events)' % (max_range, near), res, ms)

    images('the full map')
    centre = pose[:3, 3]
    before = m.num_voxels
    m.prune(box=(tuple(centre - a.box / 2), tuple(centre + a.box / 2)))
    emit('prune to a %g m box around the last pose: %d -> %d voxels' % (a.box, before, m.num_voxels))
    images('the map pruned to the box')
    emit('not measured: the split of a call between the walk arithmetic and the searches; achieved bandwidth; any counter run; how the lanes of a wave '
         'diverge when their rays end at different visits')


if __name__ == '__main__':
    main()
