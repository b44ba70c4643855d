"""Time the removal of rows from the accumulated scene cloud (include/pcacc.h C8, AccumulatedCloud.prune) on the 40-window drifting scene of
tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m), the sidecar populated as in tools/bench_accumulate_pierce.py (see_through(stamp=k)
before every add), and beside it, on the same machine and inputs, what a user does without it: the copy of the records and of the sidecar to the
host, numpy boolean masks, one np.searchsorted per offset for the neighbour count, and load() back.
  GPU leg    every figure is a whole prune() call on the final map, counter read-back included: device events around the call, one warm-up, the
             median of --repeat calls; the map is put back (not timed) before each.  Each criterion alone, stage B at r = 1 and r = 2, dry_run, and
             add of the last window before and after a prune to a --box metre box around the last pose.
  host leg   the same criteria with numpy on the copied records; stage B on the first --neighbour-rows rows (the GPU prunes the same rows for the
             comparison).  Every host result is compared with the GPU's.
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
figures give sizes and memory behaviour, not a removal rate of real ghosts.
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_prune.py [--windows 40] [--box 50] [--repeat 5] [--neighbour-rows 1000000] [--no-baseline] [--out profiles/accum_prune_bench.txt]"""
import io
import time

import numpy as np

from accum_bench import BIAS, HBM_GBS, SENSOR, Report, drift, header, parser, scene, stats, timed, voxel_coords

NAMES = ('kept', 'filter', 'stale', 'box', 'pierced', 'isolated')


class Snapshot(object):
    """The map as it stands, on the device; restore() puts it back into the cloud's current tables."""

    def __init__(self, m):
        self.n, self.capacity = m.num_voxels, m.capacity
        self.tables = tuple(t.clone() for t in m._cur)
        self.pierced, self.state = m._pierced.clone(), m._state.clone()

    def restore(self, m):
        from pcaccumulation_amd import accumulate
        if m.capacity != self.capacity or m._cur[0].shape[0] != self.capacity:
            m._cur, m._alt, m.capacity = accumulate._tables(self.capacity, m.device), None, self.capacity
        for dst, src in zip(m._cur, self.tables):
            dst.copy_(src)
        m._pierced, m._n = self.pierced.clone(), self.n
        m._state.copy_(self.state)


def host_keep(acc, min_count, max_moving_fraction):
    keep = (acc[0] >= min_count) & (acc[0] > 0)
    if max_moving_fraction is not None:
        with np.errstate(all='ignore'):
            keep &= acc[1].astype(np.float64) / acc[0].astype(np.float64) <= max_moving_fraction
    return keep


def host_neighbours(keys, radius):
    """k of every row of the ascending keys: one np.searchsorted per offset; offsets that leave the grid are masked before the key is formed."""
    c = voxel_coords(keys)
    k = np.zeros(keys.shape[0], np.int32)
    for dx in range(-radius, radius + 1):
        for dy in range(-radius, radius + 1):
            for dz in range(-radius, radius + 1):
                n = [c[0] + dx, c[1] + dy, c[2] + dz]
                ok = np.ones(keys.shape[0], bool)
                for v in n:
                    ok &= (v >= -BIAS) & (v < BIAS)
                want = ((n[0] + BIAS) << 42) | ((n[1] + BIAS) << 21) | (n[2] + BIAS)
                pos = np.minimum(np.searchsorted(keys, want), keys.shape[0] - 1)
                k += ok & (keys[pos] == want)
    return k


def parse_args(argv=None):
    ap = parser('accum_prune_bench.txt', repeat=5)
    ap.add_argument('--box', type=float, default=50.0)
    ap.add_argument('--neighbour-rows', type=int, default=1000000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--box %g --repeat %d' % (a.box, a.repeat),
                                'GPU: device events around each prune() call, counter read-back included, one warm-up, median of %d; '
                                'host: perf_counter' % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    last = None
    for k, pts, mv, T in scene(a, dev):
        m.see_through(pts, SENSOR, pose=T, moving=mv, stamp=k)
        m.add(pts, T, mv, k)
        last = (pts, mv, T)
    snap = Snapshot(m)
    total = snap.n
    centre = drift(a.windows - 1)[:3, 3]
    box = (tuple(centre - a.box / 2), tuple(centre + a.box / 2))
    emit('the map: %d voxels in tables of %d rows after %d windows, %d of them with a ray count >= 1; box: %g m around the last pose'
         % (total, snap.capacity, a.windows, int((m._pierced[:total] > 0).sum()), a.box))

    cases = [('keeps everything (min_count=1)', dict()),
             ('filter alone (min_count=2, max_moving_fraction=0.0)', dict(min_count=2, max_moving_fraction=0.0)),
             ('stale alone (before_stamp=%d)' % (a.windows // 2), dict(before_stamp=a.windows // 2)),
             ('box alone', dict(box=box)),
             ('pierced alone (min_pierced=2)', dict(min_pierced=2)),
             ('pierced with a ratio (min_pierced=2, pierced_ratio=0.5)', dict(min_pierced=2, pierced_ratio=0.5)),
             ('isolated alone, r = 1 (min_neighbors=4)', dict(min_neighbors=4, radius=1)),
             ('isolated alone, r = 2 (min_neighbors=8)', dict(min_neighbors=8, radius=2)),
             ('all together, r = 1', dict(min_count=2, max_moving_fraction=0.0, before_stamp=a.windows // 2, box=box, min_pierced=2, pierced_ratio=0.5,
                                          min_neighbors=4, radius=1))]
    gpu = {}
    for name, kw in cases:
        for dry in (False, True):
            if dry and name not in (cases[0][0], cases[-1][0], cases[6][0]):
                continue
            t = []
            for rep in range(a.repeat + 1):                                      # the first call is the warm-up
                snap.restore(m)
                torch.cuda.synchronize()
                ms, res = timed(lambda: m.prune(dry_run=dry, **kw))
                t.append(ms)
            gpu[(name, dry)] = res
            emit('GPU %s%s: %s; %s' % (name, ', dry_run' if dry else '', stats(t[1:]), ', '.join('%s %d' % (f, res[f]) for f in NAMES)))
            if name == cases[0][0] and not dry:
                gbs = 2.0 * 60.0 * total / (float(np.median(t[1:])) * 1e-3) / 1e9
                emit('  the compaction moves about 60 bytes per row each way (key 8, record 40, stamps 8, ray count 4): %.0f MB in %.2f ms = %.0f GB/s over the '
                     'WHOLE call (four kernels, the scan, a zero-fill of the new sidecar and the read-back), %.1f %% of the %.0f GB/s HBM peak'
                     % (2.0 * 60.0 * total / 1e6, float(np.median(t[1:])), gbs, 100.0 * gbs / HBM_GBS, HBM_GBS))

    # add of the last window on the full map and on the map pruned to the box
    pts, mv, T = last
    for name, kw in (('the full map', None), ('the map pruned to the box', dict(box=box))):
        t, size = [], 0
        for rep in range(a.repeat + 1):
            snap.restore(m)
            if kw is not None:
                m.prune(**kw)
            size = m.num_voxels
            torch.cuda.synchronize()
            t.append(timed(lambda: m.add(pts, T, mv, a.windows))[0])
        emit('GPU add of the last window (%d points, with the sidecar carry) on %s (%d voxels): %s' % (pts.shape[0], name, size, stats(t[1:])))

    if not a.no_baseline:
        baseline(a, torch, m, snap, box, gpu, cases, emit)
    emit('not measured: the split of a call between the stage-A kernel, the scans, the stage-B kernel and the compaction; achieved bandwidth of any single '
         'kernel; any counter run')


def baseline(a, torch, m, snap, box, gpu, cases, emit):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    snap.restore(m)
    t0 = time.perf_counter()
    keys, acc, stamps = m.records()                                              # the copies a user makes today
    pierced = m._pierced[:m.num_voxels].cpu().numpy()
    t_copy = time.perf_counter() - t0
    lo, hi = m._box_indices(box)
    inside = np.ones(keys.shape[0], bool)
    for c, l, h in zip(voxel_coords(keys), lo, hi):
        inside &= (c >= l) & (c <= h)
    masks = {cases[1][0]: lambda: host_keep(acc, 2, 0.0), cases[2][0]: lambda: stamps[1] >= a.windows // 2, cases[3][0]: lambda: inside.copy(),
             cases[4][0]: lambda: pierced < 2,
             cases[5][0]: lambda: ~((pierced >= 2) & (pierced.astype(np.float64) / acc[0].astype(np.float64) > 0.5))}
    emit('host: copy of the records and of the sidecar (%d rows) %.2f s' % (keys.shape[0], t_copy))
    for name, _ in cases[1:6]:
        t0 = time.perf_counter()
        keep = masks[name]()
        out = (keys[keep], np.ascontiguousarray(acc[:, keep]), np.ascontiguousarray(stamps[:, keep]), pierced[keep])
        t_mask = time.perf_counter() - t0
        t0 = time.perf_counter()
        buf = io.BytesIO()
        np.savez(buf, keys=out[0], acc=out[1], stamps=out[2], voxel_size=np.float64(a.voxel), dropped=np.int64(0), pierced=out[3],
                 pierce_counters=np.zeros(5, np.int64))
        buf.seek(0)
        back = AccumulatedCloud.load(buf, m.device)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        same = int(keep.sum()) == gpu[(name, False)]['kept'] == back.num_voxels
        emit('host %s: mask and compaction in numpy %.2f s, load() back %.2f s (plus the copy above); kept %d, the GPU kept %d (%s)'
             % (name, t_mask, t_load, int(keep.sum()), gpu[(name, False)]['kept'], 'equal' if same else 'DIFFERENT'))
        del back
    # stage B on the first rows only: one searchsorted per offset takes minutes on the whole map
    rows = min(a.neighbour_rows, keys.shape[0])
    buf = io.BytesIO()
    np.savez(buf, keys=keys[:rows], acc=np.ascontiguousarray(acc[:, :rows]), stamps=np.ascontiguousarray(stamps[:, :rows]), voxel_size=np.float64(a.voxel),
             dropped=np.int64(0))
    for radius, least in ((1, 4), (2, 8)):
        t0 = time.perf_counter()
        k = host_neighbours(keys[:rows], radius)
        t_host = time.perf_counter() - t0
        buf.seek(0)
        part = AccumulatedCloud.load(buf, m.device)
        t = []
        for rep in range(a.repeat + 1):
            t.append(timed(lambda: part.prune(min_neighbors=least, radius=radius, dry_run=True))[0])
        res = part.prune(min_neighbors=least, radius=radius)
        same = res['kept'] == int((k >= least).sum()) and np.array_equal(part.records()[0], keys[:rows][k >= least])
        emit('host isolated, r = %d (min_neighbors=%d), the first %d rows: %d searchsorted calls %.2f s; the GPU on the same rows (dry_run): %s; kept %d on the '
             'host, %d on the GPU, surviving keys %s' % (radius, least, rows, (2 * radius + 1) ** 3, t_host, stats(t[1:]), int((k >= least).sum()), res['kept'],
                                                          'equal' if same else 'DIFFERENT'))
        del part


if __name__ == '__main__':
    main()
