"""Time the scan-to-map registration of the accumulated scene cloud (include/pcacc.h C6, AccumulatedCloud.register) on the 40-window drifting scene
of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m) and, beside it on the same machine and inputs, what a user does without it: the
copy of the scan, the centroids and the normals to the host and a point-to-plane ICP there (scipy.spatial.cKDTree when it is installed, else the numpy
restatement tests/accumulate_register_reference.py), same gate, same update and stop rule.
  GPU leg    every window k >= 1 is registered against the map of the windows before it (init_pose = the drifting pose it comes with), then added
             with the pose it got; device events around each register call (the normals of the call and the read-back of their kept count included),
             one warm-up call; median over the windows; iterations, status and fitness per window; the voxel count of the final map with and without
             registration.
  host leg   the last window against the map before it -- one window: the host takes seconds to minutes per call.
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
scene gives the sizes and the memory behaviour of a real sequence, not a geometry that a registration could recover.  The figures are times and counts;
whether the voxel count drops says nothing about accuracy here (tests/test_accumulate_register.py has the scenes with a known pose).
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_register.py [--windows 40] [--max-iter 30] [--no-baseline] [--out profiles/accum_register_bench.txt]"""
import time

import numpy as np

from accum_bench import Report, drift, header, parser, scene, timed


def host_icp(tree, cent, nrm, pts, init, max_distance, max_iter):
    """Point-to-plane ICP on the host with a KD-tree over the centroids that have a valid normal: the contract's update and stop rule, the global
    nearest neighbour instead of the 27-voxel search.  -> pose, iterations, fitness, rmse."""
    from accumulate_register_reference import compose
    T, prev = np.array(init, np.float64), None
    for rnd in range(max_iter + 1):
        w = pts @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(w, k=1, distance_upper_bound=max_distance)
        ok = np.isfinite(d)
        nc = int(ok.sum())
        if nc == 0:
            return T, rnd, 0.0, 0.0
        wm, nm, cm = w[ok], nrm[j[ok]], cent[j[ok]]
        r = ((wm - cm) * nm).sum(1)
        fit, rmse = nc / pts.shape[0], float(np.sqrt((r * r).sum() / nc))
        if (prev is not None and abs(fit - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6) or rnd >= max_iter:
            return T, rnd, fit, rmse
        J = np.concatenate([np.cross(wm, nm), nm], 1)
        T = compose(np.linalg.solve(J.T @ J, -(J.T @ r)), T)
        prev = (fit, rmse)
    return T, max_iter, fit, rmse


def parse_args(argv=None):
    ap = parser('accum_register_bench.txt')
    ap.add_argument('--max-iter', type=int, default=30)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--max-iter %d' % a.max_iter,
                                'GPU: device events around each register call, one warm-up; host: perf_counter')).emit
    plain, reg = AccumulatedCloud(a.voxel, dev, 1 << 20), AccumulatedCloud(a.voxel, dev, 1 << 20)
    times, rows = [], []
    usable = native.REGISTER_MAX_ITER                                            # a pose that stopped at max_iter is still the best one there is
    for k, pts, mv, pose in scene(a, dev):
        plain.add(pts, pose, mv, k)
        if k:
            if k == 1:
                reg.register(pts, drift(k), mv, max_iter=a.max_iter)             # warm-up: code objects, allocator
                torch.cuda.synchronize()
            ms, res = timed(lambda: reg.register(pts, drift(k), mv, max_iter=a.max_iter))
            times.append(ms)
            status = int(res['status'])
            rows.append((k, reg.num_voxels, times[-1], int(res['iterations']), status, float(res['fitness']), float(res['rmse'])))
            if not status & ~usable:
                pose = res['pose']
            if k == a.windows - 1 and not a.no_baseline:
                baseline(a, torch, reg, pts, mv, drift(k), res, times[-1], emit)
        reg.add(pts, pose, mv, k)
    emit('GPU: %d register calls of %d points against a map of %d .. %d voxels (no filter, r = 1, max_distance = voxel): median %.2f ms, min %.2f, max %.2f; '
         'updates per call median %d (min %d, max %d); status 0 (converged) on %d calls, MAX_ITER on %d, other on %d'
         % (len(times), a.frames * a.pts_per_frame, rows[0][1], rows[-1][1], float(np.median(times)), min(times), max(times),
            int(np.median([r[3] for r in rows])), min(r[3] for r in rows), max(r[3] for r in rows), sum(r[4] == 0 for r in rows),
            sum(r[4] == usable for r in rows), sum(bool(r[4] & ~usable) for r in rows)))
    q = max(1, len(rows) // 4)
    for lo in range(0, len(rows), q):
        part = rows[lo:lo + q]
        emit('  windows %2d-%2d: map %8d -> %8d voxels, median %.2f ms; ms / updates / fitness: %s'
             % (part[0][0], part[-1][0], part[0][1], part[-1][1], float(np.median([r[2] for r in part])),
                ' '.join('%.2f/%d/%.3f' % (r[2], r[3], r[5]) for r in part)))
    emit('final map: %d voxels with the drifting poses, %d voxels with every window registered first (independent random clouds: see the docstring)'
         % (plain.num_voxels, reg.num_voxels))
    emit('not measured: the split between the correspondence and the update kernel, achieved bandwidth, any counter run; the optional sort of the scan by '
         'its voxel key was not built, so there is no figure for it')


def baseline(a, torch, reg, pts, mv, init, res, gpu_ms, emit):
    t0 = time.perf_counter()
    scan = pts.cpu().numpy()[~mv.cpu().numpy()].astype(np.float64)               # the copies a user makes today
    nrm = reg.normals()
    cent = reg.extract()['points'].cpu().numpy().astype(np.float64)
    valid = nrm['valid'].cpu().numpy()
    normals = nrm['normals'].cpu().numpy().astype(np.float64)[valid]
    cent = cent[valid]
    t_copy = time.perf_counter() - t0
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        t0 = time.perf_counter()
        tree = cKDTree(cent)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        T, iters, fit, rmse = host_icp(tree, cent, normals, scan, init, a.voxel, a.max_iter)
        t_icp = time.perf_counter() - t0
        emit('host, last window: copy of the scan, %d centroids and normals %.2f s; cKDTree build %.2f s; point-to-plane ICP %.2f s for %d updates '
             '(fitness %.3f rmse %.4f); GPU on the same call: %.2f ms for %d updates (fitness %.3f rmse %.4f); largest pose difference %.2e '
             '(global nearest neighbour on the host, 27-voxel search on the GPU: not the same correspondence rule)'
             % (cent.shape[0], t_copy, t_tree, t_icp, iters, fit, rmse, gpu_ms, int(res['iterations']), float(res['fitness']), float(res['rmse']),
                float(np.abs(T[:3] - res['pose'].cpu().numpy()[:3]).max())))
    else:
        import accumulate_reference as ref
        import accumulate_register_reference as rref
        t0 = time.perf_counter()
        r = ref.ReferenceMap(a.voxel)
        keys, acc, stamps = reg.records()
        r.rec = {int(k): [int(x) for x in acc[:, i]] + [int(stamps[0, i]), int(stamps[1, i])] for i, k in enumerate(keys)}
        want = rref.register(r, nrm['normals'].cpu().numpy(), nrm['flags'].cpu().numpy(), pts.cpu().numpy(), init, mv.cpu().numpy(), None, 1)
        emit('host, last window (no scipy here): copies %.2f s; numpy restatement, ONE update: %.1f s; GPU on the same call: %.2f ms for %d updates'
             % (t_copy, time.perf_counter() - t0, gpu_ms, int(res['iterations'])))
        del want


if __name__ == '__main__':
    main()
