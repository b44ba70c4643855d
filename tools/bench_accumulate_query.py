"""Time the per-point lookup of the accumulated scene cloud (include/pcacc.h C9, AccumulatedCloud.query) on the 40-window drifting scene of
tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m) and, beside it on the same machine and inputs, what a user does without it: the copy of
the records to the host, the float64 centroids and a nearest-neighbour search there (scipy.spatial.cKDTree when it is installed, else np.searchsorted
per offset of the 27).
  GPU leg    a fresh window of 800 000 points, under the last pose, against the full map and against the map pruned to a --box metre box around the
             last pose: query without normals (with and without extract's filter), normals() alone, query with normals=True (the normals() call and
             the read-back of its kept count included) and its share of normals(); device events around each call, one warm-up, median of --repeat.
  host leg   the full map, max_distance = 0.9 voxel (where the 27-voxel search IS the global nearest neighbour): the matched count must equal the GPU's.
The windows of this scene are independent random clouds: the scene gives the sizes and the memory behaviour of a real sequence.  The map is built by
add alone (no see_through: the kernel then reads no sidecar column).  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_query.py [--windows 40] [--box 50] [--repeat 5] [--no-baseline] [--out profiles/accum_query_bench.txt]"""
import time

import numpy as np

from accum_bench import BIAS, Report, drift, header, parser, scene, timed_repeat, window_points


def host_match(records, w, voxel, max_distance):
    """Matched points on the host: float64 centroids from the records, then a KD-tree (scipy) or the 27 offsets by np.searchsorted.  -> count, method, seconds."""
    keys, acc, _ = records
    t0 = time.perf_counter()
    cent = (acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * 2.0 ** -16
    t_cent = time.perf_counter() - t0
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        t0 = time.perf_counter()
        tree = cKDTree(cent)
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        d, _ = tree.query(w, k=1, distance_upper_bound=max_distance)
        return int(np.isfinite(d).sum()), 'cKDTree', t_cent, t_build, time.perf_counter() - t0
    t0 = time.perf_counter()
    idx = np.floor(w / voxel).astype(np.int64)
    best = np.full(w.shape[0], np.inf)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                c = idx + (dx, dy, dz)
                ok = np.all((c >= -BIAS) & (c < BIAS), 1)
                k = ((c[:, 0] + BIAS) << 42) | ((c[:, 1] + BIAS) << 21) | (c[:, 2] + BIAS)
                p = np.minimum(np.searchsorted(keys, k), keys.shape[0] - 1)
                ok &= keys[p] == k
                e = w[ok] - cent[p[ok]]
                best[ok] = np.minimum(best[ok], (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return int((best <= max_distance * max_distance).sum()), 'np.searchsorted per offset', t_cent, 0.0, time.perf_counter() - t0


def parse_args(argv=None):
    ap = parser('accum_query_bench.txt', repeat=5)
    ap.add_argument('--box', type=float, default=50.0)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--box %g --repeat %d' % (a.box, a.repeat),
                                'GPU: device events around each call, one warm-up, median of %d; host: perf_counter' % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
        if k % 10 == 9:
            print('window %d: %d voxels' % (k, m.num_voxels), flush=True)
    scan = window_points(a, a.windows, dev)                                      # a fresh window: the one after the scene's last
    pose = drift(a.windows - 1)
    n = scan.shape[0]
    filt = dict(min_count=2, max_moving_fraction=0.0)
    names = ('points', 'invalid', 'occupied', 'kept', 'matched', 'normal', 'bad_table')

    def leg(tag):
        emit('%s: %d voxels; a fresh window of %d points under the last pose' % (tag, m.num_voxels, n))
        got = {}
        for what, fn in (('query, no normals, no filter', lambda: m.query(scan, pose)),
                         ('query, no normals, min_count=2, max_moving_fraction=0.0', lambda: m.query(scan, pose, **filt)),
                         ('normals() alone, r = 1, no filter', lambda: m.normals()),
                         ('query, normals=True, no filter', lambda: m.query(scan, pose, normals=True)),
                         ('query, normals=True, require_normal=True, no filter', lambda: m.query(scan, pose, normals=True, require_normal=True))):
            res, ms = timed_repeat(fn, a.repeat)
            got[what] = float(np.median(ms))
            counts = '' if 'counters' not in res else '; ' + ', '.join('%s %d' % (k, v) for k, v in zip(names, res['counters'].tolist()))
            emit('  GPU %s: median %.3f ms, min %.3f, max %.3f%s' % (what, got[what], min(ms), max(ms), counts))
        share = got['normals() alone, r = 1, no filter'] / got['query, normals=True, no filter']
        emit('  of the call with normals=True, normals() is %.0f %%: the lookup itself takes %.3f ms with the plane distance, %.3f ms without'
             % (100 * share, got['query, normals=True, no filter'] - got['normals() alone, r = 1, no filter'], got['query, no normals, no filter']))
        return got

    full = leg('the full map')
    emit('  beside it: one register round on this scene is about 2 ms (profiles/accum_register_bench.txt: 57.46 ms median for 30 updates at 800 000 points) '
         '-- a distance, not a target: a round runs the same nine searches and sums 29 terms, the query runs a tenth search and writes ten columns')
    if not a.no_baseline:
        gate = 0.9 * a.voxel
        res, ms = timed_repeat(lambda: m.query(scan, pose, max_distance=gate), a.repeat)
        gpu_matched = int(res['counters'][native.QUERY_N_MATCHED])
        t0 = time.perf_counter()
        records = m.records()
        p = scan.cpu().numpy().astype(np.float64)
        t_copy = time.perf_counter() - t0
        w = np.stack([((pose[r, 0] * p[:, 0] + pose[r, 1] * p[:, 1]) + pose[r, 2] * p[:, 2]) + pose[r, 3] for r in range(3)], 1)
        matched, method, t_cent, t_build, t_query = host_match(records, w, a.voxel, gate)
        emit('host, the full map, max_distance = 0.9 voxel: copy of the records and the scan %.2f s; float64 centroids %.2f s; %s: build %.2f s, query %.2f s; '
             'matched %d; GPU on the same call: median %.3f ms, matched %d' % (t_copy, t_cent, method, t_build, t_query, matched, float(np.median(ms)), gpu_matched))
        assert matched == gpu_matched, (matched, gpu_matched)
    centre = pose[:3, 3]
    before = m.num_voxels
    m.prune(box=(tuple(centre - a.box / 2), tuple(centre + a.box / 2)))
    emit('prune to a %g m box around the last pose: %d -> %d voxels' % (a.box, before, m.num_voxels))
    leg('the map pruned to the box')
    del full
    emit('not measured: the achieved bandwidth of the kernel, any counter run; the optional sort of the scan by its voxel key was not built, so there is no '
         'figure for it')


if __name__ == '__main__':
    main()
