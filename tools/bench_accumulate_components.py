"""Time the connected components of the accumulated scene cloud (include/pcacc.h C11, AccumulatedCloud.components / remove_components) on the
40-window drifting scene of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m), and beside it, on the same machine and keys, what a user
does without it: the copy of the keys to the host, one np.searchsorted per offset for the edges and scipy.sparse.csgraph.connected_components.
  GPU leg    every figure is a whole call on the final map, counter read-back included: device events around the call, one warm-up, the median of
             --repeat calls; K and the largest component stand next to each time.  components() at r = 1 and r = 2 with and without the filter,
             remove_components(min_voxels) with the map put back (not timed) before each call.
  host leg   on the first --host-rows rows of the map (the whole map takes minutes): edges from the 13 (r = 1) offsets with smaller keys, scipy's
             labels renumbered by first occurrence -- the contract's order -- and compared with the GPU's labels on a map of the same rows.
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
figures give sizes and memory behaviour, not the component structure of a real drive.
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_components.py [--windows 40] [--repeat 5] [--min-voxels 10] [--host-rows 1000000] [--no-baseline]
       [--out profiles/accum_components_bench.txt]"""
import io
import time

import numpy as np

from accum_bench import BIAS, Report, header, parser, scene, stats, timed, voxel_coords


def host_labels(keys, radius):
    """Labels of the ascending keys, every row taking part: edges to the offsets with smaller keys (one np.searchsorted each; offsets that leave the
    grid are masked before the key is formed), scipy's components, renumbered in ascending order of their first row."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = keys.shape[0]
    c = voxel_coords(keys)
    src, dst = [], []
    for dx in range(-radius, radius + 1):
        for dy in range(-radius, radius + 1):
            for dz in range(-radius, radius + 1):
                if (dx, dy, dz) >= (0, 0, 0):
                    continue
                v = [c[0] + dx, c[1] + dy, c[2] + dz]
                ok = np.ones(n, bool)
                for a in v:
                    ok &= (a >= -BIAS) & (a < BIAS)
                want = ((v[0] + BIAS) << 42) | ((v[1] + BIAS) << 21) | (v[2] + BIAS)
                pos = np.minimum(np.searchsorted(keys, want), n - 1)
                hit = ok & (keys[pos] == want)
                src.append(np.nonzero(hit)[0])
                dst.append(pos[hit])
    src, dst = np.concatenate(src), np.concatenate(dst)
    k, lab = connected_components(coo_matrix((np.ones(src.shape[0], np.int8), (src, dst)), shape=(n, n)), directed=False)
    _, first = np.unique(lab, return_index=True)
    order = np.empty(k, np.int64)
    order[np.argsort(first)] = np.arange(k)
    return order[lab].astype(np.int32), k, src.shape[0]


def parse_args(argv=None):
    ap = parser('accum_components_bench.txt', repeat=5)
    ap.add_argument('--min-voxels', type=int, default=10)
    ap.add_argument('--host-rows', type=int, default=1000000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--repeat %d --min-voxels %d' % (a.repeat, a.min_voxels),
                                'GPU: device events around each call, counter read-back included, one warm-up, median of %d; host: perf_counter'
                                % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
    total = m.num_voxels
    tables, state = tuple(t.clone() for t in m._cur), m._state.clone()
    emit('the map: %d voxels in tables of %d rows after %d windows' % (total, m.capacity, a.windows))

    def restore():
        for dst, src in zip(m._cur, tables):
            dst.copy_(src)
        m._n = total
        m._state.copy_(state)

    for name, kw in (('r = 1', dict(radius=1)), ('r = 2', dict(radius=2)), ('r = 1, min_count=2, max_moving_fraction=0.0', dict(radius=1, min_count=2, max_moving_fraction=0.0)),
                     ('r = 2, min_count=2, max_moving_fraction=0.0', dict(radius=2, min_count=2, max_moving_fraction=0.0))):
        t = []
        for rep in range(a.repeat + 1):                                          # the first call is the warm-up
            ms, res = timed(lambda: m.components(**kw))
            t.append(ms)
        c = res['counters'].tolist()
        emit('GPU components(%s): %s; %d rows take part, K %d, largest component %d voxels' % (name, stats(t[1:]), c[native.COMPONENTS_PARTICIPATING],
                                                                                             c[native.COMPONENTS_K], c[native.COMPONENTS_LARGEST]))
    for name, kw in (('r = 1', dict(radius=1)), ('r = 2', dict(radius=2))):
        for dry in (False, True):
            t = []
            for rep in range(a.repeat + 1):
                restore()
                torch.cuda.synchronize()
                ms, res = timed(lambda: m.remove_components(min_voxels=a.min_voxels, dry_run=dry, **kw))
                t.append(ms)
            emit('GPU remove_components(min_voxels=%d, %s%s): %s; kept %d, small %d, components removed %d, kept %d, largest %d'
                 % (a.min_voxels, name, ', dry_run' if dry else '', stats(t[1:]), res['kept'], res['small'], res['components_removed'], res['components_kept'],
                    res['largest']))
    restore()
    if not a.no_baseline:
        t0 = time.perf_counter()
        keys = m.records()[0]
        t_copy = time.perf_counter() - t0
        rows = min(a.host_rows, keys.shape[0])
        emit('host: copy of the records (%d rows) %.2f s; the baseline below runs on the first %d rows' % (keys.shape[0], t_copy, rows))
        buf = io.BytesIO()
        acc, stamps = m.records()[1], m.records()[2]
        np.savez(buf, keys=keys[:rows], acc=np.ascontiguousarray(acc[:, :rows]), stamps=np.ascontiguousarray(stamps[:, :rows]), voxel_size=np.float64(a.voxel),
                 dropped=np.int64(0))
        for radius in (1, 2):
            t0 = time.perf_counter()
            lab, k, n_edges = host_labels(keys[:rows], radius)
            t_host = time.perf_counter() - t0
            buf.seek(0)
            part = AccumulatedCloud.load(buf, dev)
            t = []
            for rep in range(a.repeat + 1):
                ms, res = timed(lambda: part.components(radius=radius))
                t.append(ms)
            same = np.array_equal(res['label'].cpu().numpy(), lab) and k == int(res['counters'][native.COMPONENTS_K])
            assert same, 'the labels of the host baseline and of the GPU differ at r = %d' % radius
            emit('host r = %d, the first %d rows: %d searchsorted calls and scipy connected_components over %d edges %.2f s, K %d; the GPU on the same rows: '
                 '%s; labels equal' % (radius, rows, ((2 * radius + 1) ** 3 - 1) // 2, n_edges, t_host, k, stats(t[1:])))
            del part
    emit('not measured: the split of a call between the row table, link, flatten, numbering and statistics kernels; the cost of contention on a giant '
         'component (atomicCAS retries, the depth of the trees before flatten); any counter run')


if __name__ == '__main__':
    main()
