"""Time the per-voxel normals of the accumulated scene cloud (include/pcacc.h C5, AccumulatedCloud.normals) on the 40-window drifting scene of
tools/bench_accumulate.py (8 M voxels at 0.1 m) and, beside it on the same machine, what a user does without it: the copy of the map's records to
the host and a vectorised numpy PCA there (np.searchsorted on the copied keys for every offset of the neighbourhood, float64 sums, np.linalg.eigh).
  GPU legs   r = 1 and r = 2, without a filter and under extract's min_count=2, max_moving_fraction=0.0; device events around the call (kernels and
             the read-back of the kept count included), one warm-up call, median of 5.
  host leg   on the sub-map of the first --baseline-rows rows (a slab in x: the keys ascend in x) -- the full map takes minutes per radius on the
             host -- with the GPU timed on the same sub-map; neighbour counts are compared for equality, normals up to sign.
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_normals.py [--windows 40] [--baseline-rows 1000000] [--no-baseline] [--out profiles/accum_normals_bench.txt]"""
import os
import tempfile
import time

import numpy as np

from accum_bench import BIAS, Report, drift, header, parser, scene, timed_repeat, voxel_coords

FILTERS = (('no filter', dict()), ('min_count=2, max_moving_fraction=0.0', dict(min_count=2, max_moving_fraction=0.0)))


def host_normals(keys, acc, radius, min_neighbors, min_count=1, max_moving_fraction=None):
    """The contract in vectorised numpy on host records: one np.searchsorted per offset, in key order.  -> neighbors, flags & 3, normals (unsigned)."""
    keep = (acc[0] >= min_count) & (acc[0] > 0)
    if max_moving_fraction is not None:
        keep &= acc[1].astype(np.float64) / np.maximum(acc[0], 1).astype(np.float64) <= max_moving_fraction
    k = keys[keep]
    cent = (acc[2:5, keep].T.astype(np.float64) / acc[0, keep].astype(np.float64)[:, None]) * 2.0 ** -16
    v = k.shape[0]
    c = voxel_coords(k)
    n = np.zeros(v, np.int32)
    s1, s2 = np.zeros((v, 3)), np.zeros((v, 6))
    rng = range(-radius, radius + 1)
    for dx in rng:
        for dy in rng:
            for dz in rng:
                q = [c[0] + dx, c[1] + dy, c[2] + dz]
                ok = np.ones(v, bool)
                for a in q:
                    ok &= (a >= -BIAS) & (a < BIAS)
                qk = np.where(ok, ((q[0] + BIAS) << 42) | ((q[1] + BIAS) << 21) | (q[2] + BIAS), 0)
                p = np.minimum(np.searchsorted(k, qk), max(v - 1, 0))
                hit = ok & (k[p] == qk)
                d = np.where(hit[:, None], cent[p] - cent, 0.0)
                n += hit
                s1 += d
                s2 += np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    mu = s1 / n[:, None]
    cov = np.empty((v, 3, 3))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        cov[:, a, b] = cov[:, b, a] = s2[:, j] / n - mu[:, a] * mu[:, b]
    w, vec = np.linalg.eigh(cov)
    w = np.maximum(w, 0.0)
    flags = (n < min_neighbors).astype(np.uint8) | ((w[:, 1] <= 64 * 2.0 ** -52 * w[:, 2]).astype(np.uint8) << 1)
    with np.errstate(all='ignore'):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return n, flags, vec[:, :, 0], gap


def parse_args(argv=None):
    ap = parser('accum_normals_bench.txt')
    ap.add_argument('--baseline-rows', type=int, default=1000000)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--baseline-rows %d' % a.baseline_rows,
                                'GPU: device events around each call, median of 5 after one warm-up; host: perf_counter')).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
    viewpoints = torch.from_numpy(np.stack([drift(k)[:3, 3] for k in range(a.windows)])).to(dev)
    emit('map: %d windows -> %d voxels (capacity %d)' % (a.windows, m.num_voxels, m.capacity))

    def report(cloud, what):
        for fname, f in FILTERS:
            for radius in (1, 2):
                out, times = timed_repeat(lambda: cloud.normals(radius=radius, viewpoints=viewpoints, **f), 5)
                emit('GPU %s, %s, r = %d: %d rows, %d valid, mean k %.1f; median %.2f ms (%s)'
                     % (what, fname, radius, out['flags'].shape[0], int(out['valid'].sum()), float(out['neighbors'].float().mean()),
                        float(np.median(times)), ' '.join('%.2f' % t for t in times)))

    report(m, 'full map')
    if not a.no_baseline and m.num_voxels:
        rows = min(a.baseline_rows, m.num_voxels)
        keys, acc, stamps = m.records()
        with tempfile.TemporaryDirectory() as tmp:                               # the sub-map as a map of its own, through the public save format
            path = os.path.join(tmp, 'sub.npz')
            np.savez(path, keys=keys[:rows], acc=np.ascontiguousarray(acc[:, :rows]), stamps=np.ascontiguousarray(stamps[:, :rows]),
                     voxel_size=np.float64(a.voxel), dropped=np.int64(0))
            sub = AccumulatedCloud.load(path, dev)
        del keys, acc, stamps
        report(sub, 'sub-map of the first %d rows' % rows)
        for fname, f in FILTERS:
            for radius in (1, 2):
                got = sub.normals(radius=radius, **f)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hk, ha, _ = sub.records()                                        # the copy a user makes today, then the PCA in numpy
                n, flags, nrm, gap = host_normals(hk, ha, radius, 5, **f)
                t_host = time.perf_counter() - t0
                g_n, g_flags = got['neighbors'].cpu().numpy(), got['flags'].cpu().numpy()
                clear = (flags == 0) & (gap >= 1e-3)
                g_nrm = got['normals'].cpu().numpy().astype(np.float64)[clear]
                diff = np.abs(np.abs((g_nrm * nrm[clear]).sum(1)) - 1.0).max() if clear.any() else 0.0
                emit('host sub-map, %s, r = %d: copy + numpy (searchsorted per offset, eigh) %.1f s for %d rows; neighbours equal: %s; '
                     'flags equal: %s; largest |1 - |n_gpu . n_host|| on the %d valid rows with gap >= 1e-3: %.2g'
                     % (fname, radius, t_host, n.shape[0], bool(np.array_equal(n, g_n)), bool(np.array_equal(flags, g_flags & 3)),
                        int(clear.sum()), diff))


if __name__ == '__main__':
    main()
