"""Time the planar segments of the accumulated scene cloud (include/pcacc.h C18, AccumulatedCloud.planes / split_planes) on the 40-window drifting
scene of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m), and beside it, on the same machine and inputs, what a user does without it:
the copy of the records and the normals to the host, the gated edges by one np.searchsorted per offset and scipy.sparse.csgraph.connected_components.
  GPU leg    every figure is a whole call on the final map, counter read-back included: device events around the call, one warm-up, the median of
             --repeat calls with min and max; the counters stand next to each time.  planes() with given normals, planes() with its normals() call
             included, split_planes().
  host leg   once, on the first --host-rows rows of the map (the whole map takes minutes): the rows that take part from the flags and the flatness
             product, edges from the 13 offsets with smaller keys gated by the contract's rule in numpy float64 in its order of operations, scipy's
             labels renumbered by first row and asserted equal to the GPU's labels on a map of the same rows.
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
figures give sizes and memory behaviour, not the segment structure of a real drive; few rows are flat, so max_variation 1 (no gate) is timed as well.
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_planes.py [--windows 40] [--repeat 5] [--host-rows 1000000] [--no-baseline] [--out profiles/accum_planes_bench.txt]"""
import io
import math
import time

import numpy as np

from accum_bench import BIAS, Report, header, parser, scene, timed_repeat, voxel_coords


def host_labels(keys, acc, normals, eigenvalues, flags, cos_angle, max_offset, max_variation):
    """Labels [n] (-1: the row takes no part) by the contract's rule at radius 1, every array over the same rows: scipy's components renumbered in
    ascending order of their first row.  -> labels, K, edges."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = keys.shape[0]
    e = eigenvalues.astype(np.float64)
    part = ((flags & 3) == 0) & (e[:, 2] <= np.float64(max_variation) * ((e[:, 0] + e[:, 1]) + e[:, 2]))
    nrm = normals.astype(np.float64)
    cen = (acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * np.float64(2.0 ** -16)
    c = voxel_coords(keys)
    src, dst = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) >= (0, 0, 0):
                    continue
                v = [c[0] + dx, c[1] + dy, c[2] + dz]
                ok = part.copy()
                for a in v:
                    ok &= (a >= -BIAS) & (a < BIAS)
                want = ((v[0] + BIAS) << 42) | ((v[1] + BIAS) << 21) | (v[2] + BIAS)
                pos = np.minimum(np.searchsorted(keys, want), n - 1)
                i = np.nonzero(ok & (keys[pos] == want) & part[pos])[0]
                p = pos[i]
                a, b, d = nrm[i], nrm[p], cen[p] - cen[i]
                dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
                off_a = (a[:, 0] * d[:, 0] + a[:, 1] * d[:, 1]) + a[:, 2] * d[:, 2]
                off_b = (b[:, 0] * d[:, 0] + b[:, 1] * d[:, 1]) + b[:, 2] * d[:, 2]
                hit = (np.abs(dot) >= cos_angle) & (np.abs(off_a) <= max_offset) & (np.abs(off_b) <= max_offset)
                src.append(i[hit])
                dst.append(p[hit])
    src, dst = np.concatenate(src), np.concatenate(dst)
    _, lab = connected_components(coo_matrix((np.ones(src.shape[0], np.int8), (src, dst)), shape=(n, n)), directed=False)
    lab = np.where(part, lab, -1)
    uniq, first = np.unique(lab[part], return_index=True)
    order = np.full(int(lab.max()) + 2, -1, np.int64)
    order[uniq[np.argsort(first)]] = np.arange(uniq.shape[0])
    return np.where(part, order[np.maximum(lab, 0)], -1).astype(np.int32), uniq.shape[0], src.shape[0]


def parse_args(argv=None):
    ap = parser('accum_planes_bench.txt', repeat=5)
    ap.add_argument('--host-rows', type=int, default=1000000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--repeat %d' % a.repeat,
                                'GPU: device events around each call, counter read-back included, one warm-up, median of %d; host: perf_counter, once'
                                % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
        if k % 10 == 9:
            print('window %d: %d voxels' % (k, m.num_voxels), flush=True)
    emit('the map: %d voxels in tables of %d rows after %d windows; normals at radius 2, min_neighbors 5' % (m.num_voxels, m.capacity, a.windows))
    names = ('rows', 'take part', 'outside', 'masked', 'no valid normal', 'not flat', 'K', 'largest', 'status')

    def report(what, fn, counters=lambda res: res['counters']):
        res, ms = timed_repeat(fn, a.repeat)
        counts = '' if counters is None else '; ' + ', '.join('%s %d' % (k, v) for k, v in zip(names, counters(res).tolist()))
        emit('  GPU %s: median %.3f ms, min %.3f, max %.3f%s' % (what, float(np.median(ms)), min(ms), max(ms), counts))
        return res

    nrm, ms = timed_repeat(lambda: m.normals(radius=2, min_neighbors=5), a.repeat)
    emit('  GPU normals(radius=2) alone, for scale: median %.3f ms, min %.3f, max %.3f' % (float(np.median(ms)), min(ms), max(ms)))
    for mv in (0.01, 1.0):
        report('planes(max_variation=%g) with given normals' % mv, lambda: m.planes(max_variation=mv, normals=nrm))
        report('planes(max_variation=%g) including its normals() call' % mv, lambda: m.planes(max_variation=mv))
    res = m.planes(max_variation=1.0, normals=nrm)
    min_voxels = 50
    pair = report('split_planes(min_voxels=%d, max_variation=1), its planes() call (normals given) and the two select() calls included' % min_voxels,
                  lambda: m.split_planes(min_voxels, max_variation=1.0, normals=nrm), None)
    emit('  segments of at least %d voxels: %d; the two maps hold %d + %d voxels' % (min_voxels, int((res['voxels'] >= min_voxels).sum()), pair[0].num_voxels,
                                                                                   pair[1].num_voxels))
    if not a.no_baseline:
        t0 = time.perf_counter()
        keys, acc, stamps = m.records()
        host_n = [nrm[f].cpu().numpy() for f in ('normals', 'eigenvalues', 'flags')]
        t_copy = time.perf_counter() - t0
        rows = min(a.host_rows, keys.shape[0])
        emit('host: copy of the records and the normals (%d rows) %.2f s; the baseline below runs on the first %d rows' % (keys.shape[0], t_copy, rows))
        buf = io.BytesIO()
        np.savez(buf, keys=keys[:rows], acc=np.ascontiguousarray(acc[:, :rows]), stamps=np.ascontiguousarray(stamps[:, :rows]), voxel_size=np.float64(a.voxel),
                 dropped=np.int64(0))
        buf.seek(0)
        part = AccumulatedCloud.load(buf, dev)
        part_n = part.normals(radius=2, min_neighbors=5)                         # the normals of the part map: both legs read the same arrays
        arrays = [part_n[f].cpu().numpy() for f in ('normals', 'eigenvalues', 'flags')]
        cos_angle, max_offset = math.cos(math.radians(15.0)), 0.5 * a.voxel
        for mv in (0.01, 1.0):
            t0 = time.perf_counter()
            lab, k, n_edges = host_labels(keys[:rows], acc[:, :rows], arrays[0], arrays[1], arrays[2], cos_angle, max_offset, mv)
            t_host = time.perf_counter() - t0
            got, ms = timed_repeat(lambda: part.planes(max_variation=mv, normals=part_n), a.repeat)
            same = np.array_equal(got['label'].cpu().numpy(), lab) and k == int(got['counters'][native.PLANES_K])
            assert same, 'the labels of the host baseline and of the GPU differ at max_variation %g' % mv
            emit('host max_variation=%g, the first %d rows: 13 searchsorted calls, the gate and scipy connected_components over %d edges %.2f s, K %d; the GPU '
                 'on the same rows: median %.3f ms, min %.3f, max %.3f; labels equal' % (mv, rows, n_edges, t_host, k, float(np.median(ms)), min(ms), max(ms)))
        del host_n
    emit('not measured: the split of a call between the row table, class, link, flatten, numbering, the two statistics passes, fit and distance kernels; '
         'the cost of contention on a giant segment (atomicCAS retries, the depth of the trees before flatten, the atomics of the run totals); any counter run')


if __name__ == '__main__':
    main()
