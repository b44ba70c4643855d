"""Time the distance field of the accumulated scene cloud (include/pcacc.h C19, AccumulatedCloud.distance_field / clearance) on the 40-window drifting scene
of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m) and, beside it on the same machine and inputs, what a user does without it: the copy of
the records to the host and scipy.ndimage.distance_transform_edt of the same box.
  GPU leg    distance_field() of a 512 x 512 x 64 box around the median voxel of the map (pad=False: the box itself) at max_radius 8, 32 and 128, and its
             planar form, the read-back of the counters included; clearance() of 800 000 points against the field of R = 32; device events around
             each call, one warm-up, median of --repeat with min and max.  (The recorded profiles/accum_field_bench.txt comes from the revision of this
             tool that also timed an LDS-tiled form of the y / x passes, which lost and was removed: DESIGN.md section 9s.)
  host leg   once: records() (the copy), the occupancy grid of the box, scipy.ndimage.distance_transform_edt, squared and rounded; dist2 must equal the
             GPU's wherever d2 <= R^2, and the GPU's must be -1 elsewhere.
The windows of this scene are independent random clouds: the scene gives the sizes and the memory behaviour of a real sequence.  Results go to --out.
Nothing is gated on the times.
Usage: python tools/bench_accumulate_field.py [--windows 40] [--repeat 5] [--no-baseline] [--out profiles/accum_field_bench.txt]"""
import time

import numpy as np

from accum_bench import Report, header, parser, scene, timed_repeat, voxel_coords


def parse_args(argv=None):
    ap = parser('accum_field_bench.txt', repeat=5)
    ap.add_argument('--box', type=int, nargs=3, default=(512, 512, 64))
    ap.add_argument('--points', type=int, default=800000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--repeat %d --box %d %d %d' % ((a.repeat,) + tuple(a.box)),
                                'GPU: device events around each call, one warm-up, median of %d; host: perf_counter, once' % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
    coords = m.extract()['coords']
    centre = coords.median(0).values.tolist()
    shape = tuple(a.box)
    origin = tuple(int(c) - n // 2 for c, n in zip(centre, shape))
    emit('the full map: %d voxels, no filter; the box: origin %r, shape %r = %d cells (planar: %d), pad=False' % ((m.num_voxels, origin, shape,
                                                                                                                 shape[0] * shape[1] * shape[2], shape[0] * shape[1])))
    names = ('rows', 'sites', 'cells with a result', 'cells without')
    fields = {}
    for planar in (False, True):
        for R in (8, 32, 128):
            def call():
                f = m.distance_field(origin, shape, R, planar, pad=False)
                f['counts'] = f['counters'].tolist()                             # the read-back
                return f
            fields[(planar, R)], ms = timed_repeat(call, a.repeat)
            emit('  GPU distance_field(max_radius=%d, planar=%s): median %.3f ms, min %.3f, max %.3f; %s'
                 % (R, planar, float(np.median(ms)), min(ms), max(ms), ', '.join('%s %d' % (k, v) for k, v in zip(names, fields[(planar, R)]['counts']))))
    lo = torch.tensor(origin, dtype=torch.float64) * a.voxel
    pts = (lo + torch.rand((a.points, 3), dtype=torch.float64) * torch.tensor(shape, dtype=torch.float64) * a.voxel * 1.1).float().to(dev)
    for planar in (False, True):
        def look():
            out = m.clearance(points=pts, field=fields[(planar, 32)])
            out['counts'] = out['counters'].tolist()
            return out
        out, ms = timed_repeat(look, a.repeat)
        emit('  GPU clearance of %d points against the field of R = 32, planar=%s, the read-back of the counters included: median %.3f ms, min %.3f, max %.3f; '
             'rows %d, valid %d, inside %d, near %d' % ((a.points, planar, float(np.median(ms)), min(ms), max(ms)) + tuple(out['counts'])))
    if not a.no_baseline:
        from scipy.ndimage import distance_transform_edt
        t0 = time.perf_counter()
        keys, _, _ = m.records()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        c = np.stack(voxel_coords(keys), 1) - np.array(origin)
        c = c[np.all((c >= 0) & (c < np.array(shape)), 1)]
        occ = np.zeros(shape, bool)
        occ[tuple(c.T)] = True
        t_grid = time.perf_counter() - t0
        t0 = time.perf_counter()
        edt = np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64)
        t_edt = time.perf_counter() - t0
        t0 = time.perf_counter()
        flat = np.rint(distance_transform_edt(~occ.any(2)) ** 2).astype(np.int64)
        t_flat = time.perf_counter() - t0
        same = True
        for (planar, R), f in sorted(fields.items()):
            got, want = f['dist2'].cpu().numpy().astype(np.int64), (flat[:, :, None] if planar else edt)
            same &= bool(np.array_equal(got, np.where(want <= R * R, want, -1)))
        emit('host, the same box: copy of the records %.2f s; the occupancy grid %.2f s (%d voxels inside); scipy.ndimage.distance_transform_edt %.2f s '
             '(untruncated, no nearest row), of the planar grid %.2f s; dist2 where d2 <= R^2 and -1 elsewhere are %s to the GPU\'s at every R, both forms'
             % (t_copy, t_grid, int(occ.sum()), t_edt, t_flat, 'equal' if same else 'NOT equal'))
        assert same
    emit('not measured here: the split between pass 1, the memset, the site kernel and the three passes, the achieved bandwidth, any counter run, other '
         'scenes, other boxes, a filter; the lower-envelope transform was not built, so there is no A/B against it')


if __name__ == '__main__':
    main()
