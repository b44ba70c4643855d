"""Time the k-nearest search of the accumulated scene cloud (include/pcacc.h C16, AccumulatedCloud.knn / neighbors) on the 40-window drifting scene of
tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m) and, beside it on the same machine and inputs, what a user does without it: the copy of
the records to the host, the float64 centroids and scipy.spatial.cKDTree there (when scipy is installed).
  GPU leg    a fresh window of 800 000 points, under the last pose, against the full map: query() (C9, the comparable call that was there before) and
             knn at (k, r) = (1, 1), (8, 2), (16, 3) and (16, 4); then neighbors(8, 2) on the map pruned to a --box metre box around the last pose;
             device events around each call, one warm-up, median of --repeat.
  host leg   the full map, k = 8, max_distance = 1.9 voxels (where the 5^3 block search IS the global k nearest): the neighbour sets must equal the GPU's.
The windows of this scene are independent random clouds: the scene gives the sizes and the memory behaviour of a real sequence.  Results go to --out.
Nothing is gated on them.  An A/B of two builds of the library runs this tool alternately with PCACC_LIB naming the other build (the appendix of
profiles/accum_knn_bench.txt was made that way, with --no-baseline).
Usage: python tools/bench_accumulate_knn.py [--windows 40] [--box 50] [--repeat 5] [--no-baseline] [--out profiles/accum_knn_bench.txt]"""
import time

import numpy as np

from accum_bench import Report, drift, header, parser, scene, timed_repeat, window_points


def parse_args(argv=None):
    ap = parser('accum_knn_bench.txt', repeat=5)
    ap.add_argument('--box', type=float, default=50.0)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
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
    names = ('queries', 'invalid', 'found', 'full', 'neighbours')

    def report(what, fn):
        res, ms = timed_repeat(fn, a.repeat)
        counts = ', '.join('%s %d' % (k, v) for k, v in zip(names, res['counters'].tolist())) if res['counters'].numel() == 5 else \
            'matched %d' % int(res['counters'][4])
        emit('  GPU %s: median %.3f ms, min %.3f, max %.3f; %s' % (what, float(np.median(ms)), min(ms), max(ms), counts))
        return res, float(np.median(ms))

    emit('the full map: %d voxels; a fresh window of %d points under the last pose, no filter' % (m.num_voxels, n))
    _, t_query = report('query(), C9: one neighbour within one voxel, ten columns', lambda: m.query(scan, pose))
    _, t_11 = report('knn(k=1, radius=1)', lambda: m.knn(scan, 1, pose, radius=1))
    for k, r in ((8, 2), (16, 3), (16, 4)):
        report('knn(k=%d, radius=%d)' % (k, r), lambda: m.knn(scan, k, pose, radius=r))
    emit('  knn(1, 1) beside query(): %.3f ms against %.3f ms -- a distance, not a target: the same nine columns; query runs a tenth search for '
         'the own voxel and writes ten columns, knn writes four' % (t_11, t_query))
    if not a.no_baseline:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is None:
            emit('host: scipy is not installed: no cKDTree figure')
        else:
            gate = 1.9 * a.voxel
            res, t_gpu = report('knn(k=8, radius=2, max_distance=1.9 voxels)', lambda: m.knn(scan, 8, pose, radius=2, max_distance=gate))
            t0 = time.perf_counter()
            _, acc, _ = m.records()
            p = scan.cpu().numpy().astype(np.float64)
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            cent = (acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * 2.0 ** -16
            w = np.stack([((pose[r, 0] * p[:, 0] + pose[r, 1] * p[:, 1]) + pose[r, 2] * p[:, 2]) + pose[r, 3] for r in range(3)], 1)
            t_cent = time.perf_counter() - t0
            t0 = time.perf_counter()
            tree = cKDTree(cent)
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            d, j = tree.query(w, k=8, distance_upper_bound=gate)
            t_tree = time.perf_counter() - t0
            host = np.sort(np.where(np.isfinite(d), j, -1), 1)                   # without a filter extract's row is the map row: the tree's index
            same = np.array_equal(host, np.sort(res['rows'].cpu().numpy(), 1))
            emit('host, the full map, k = 8, max_distance = 1.9 voxels: copy of the records and the scan %.2f s; float64 centroids and world points %.2f s; '
                 'cKDTree: build %.2f s, query %.2f s; neighbours %d; GPU on the same call: median %.3f ms, neighbours %d; the neighbour sets are %s'
                 % (t_copy, t_cent, t_build, t_tree, int(np.isfinite(d).sum()), t_gpu, int(res['counters'][4]), 'equal' if same else 'NOT equal'))
            assert same
    centre = pose[:3, 3]
    before = m.num_voxels
    m.prune(box=(tuple(centre - a.box / 2), tuple(centre + a.box / 2)))
    emit('prune to a %g m box around the last pose: %d -> %d voxels' % (a.box, before, m.num_voxels))
    report('neighbors(k=8, radius=2), every row of the pruned map, the read-back of the kept count included', lambda: m.neighbors(8, radius=2))
    report('knn(k=8, radius=2), the fresh window against the pruned map', lambda: m.knn(scan, 8, pose, radius=2))
    emit('not measured: the achieved bandwidth of the kernels, any counter run, other scenes; a lane group per query was not built, so there is no A/B '
         'for it')


if __name__ == '__main__':
    main()
