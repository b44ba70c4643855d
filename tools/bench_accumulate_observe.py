"""Time the observed-space table (include/pcacc.h C14, ObservedSpace.observe / lookup) on the 40-window drifting scene of tools/bench_accumulate.py
(5 x 160 k points per window, the sensor 1.8 m above the window's origin) and, beside it in the same session and on the same rays, see_through (C7),
which does a different job: a search per visit and no sort.
  every window runs observe(stamp=k) into the space, then see_through(stamp=k) against the cloud of the windows before it, then add(stamp=k); device
  events around each call (an observe call includes its read-backs of the state words and every attempt: the cut for the visit budget, the growth of
  the tables), one warm-up; max_steps 4096; once at --voxel and once at --coarse.  Then lookup() of the last window's points, --repeats times.
The windows of this scene are INDEPENDENT random clouds (synthetic.make_sequence draws range points along the beams of a sensor, not surfaces): the
figures give sizes and memory behaviour, not a free-space rate (tests/test_accumulate_observe.py has the scene with a known answer).
Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_observe.py [--windows 40] [--voxel 0.1] [--coarse 0.4] [--out profiles/accum_observe_bench.txt]"""
import numpy as np

from accum_bench import SENSOR, Report, header, parser, scene, stats, timed


def parse_args(argv=None):
    ap = parser('accum_observe_bench.txt', repeats=10, baseline=False)
    ap.add_argument('--coarse', type=float, default=0.4)
    ap.add_argument('--max-steps', type=int, default=4096)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud, ObservedSpace, _observe_chunks
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--coarse %g --max-steps %d' % (a.coarse, a.max_steps),
                                'device events around each call, one warm-up')).emit
    windows = []
    for k, pts, mv, T in scene(a, dev):
        windows.append((pts, mv, T))
        if k % 10 == 9:
            print('scene: %d windows built' % (k + 1), flush=True)
    n = windows[0][0].shape[0]
    warm_c, warm_s = AccumulatedCloud(a.voxel, dev, 1 << 20), ObservedSpace(a.voxel, dev)      # warm-up: code objects, allocator, the sort's first call
    warm_c.add(windows[0][0], windows[0][2], windows[0][1], 0)
    warm_c.see_through(windows[0][0], SENSOR, pose=windows[0][2], moving=windows[0][1], stamp=1, max_steps=a.max_steps)
    warm_s.observe(windows[0][0], SENSOR, pose=windows[0][2], moving=windows[0][1], stamp=0, max_steps=a.max_steps)
    warm_s.lookup(windows[0][0], windows[0][2])
    budget = warm_s.visit_budget
    del warm_c, warm_s
    torch.cuda.synchronize()
    first = _observe_chunks(n, a.max_steps)[0]
    emit('workspace of one call at the default visit budget 2^%d: %d bytes for the first %d rays of a window (visit_capacity = the budget), '
         '%d bytes for a piece of 100000 rays; of it %d bytes per visit of capacity'
         % (budget.bit_length() - 1, native.accum_observe_workspace_bytes(first[1] - first[0], budget), first[1] - first[0],
            native.accum_observe_workspace_bytes(100000, budget),
            (native.accum_observe_workspace_bytes(100000, budget) - native.accum_observe_workspace_bytes(100000, budget // 2)) // (budget // 2)))

    for vs in (a.voxel, a.coarse):
        cloud, sp = AccumulatedCloud(vs, dev, 1 << 20), ObservedSpace(vs, dev)
        t_obs, t_see, visits, splits, sizes, caps = [], [], [], [], [], []
        for k, (pts, mv, T) in enumerate(windows):
            v0, s0 = sp.counters['visits'], sp.splits
            t_obs.append(timed(lambda: sp.observe(pts, SENSOR, pose=T, moving=mv, stamp=k, max_steps=a.max_steps))[0])
            visits.append(sp.counters['visits'] - v0)
            splits.append(sp.splits - s0)
            sizes.append(sp.num_voxels)
            caps.append(sp.capacity)
            t_see.append(timed(lambda: cloud.see_through(pts, SENSOR, pose=T, moving=mv, stamp=k, max_steps=a.max_steps))[0])
            cloud.add(pts, T, mv, k)
        c = sp.counters
        grew = [k for k in range(1, len(caps)) if caps[k] != caps[k - 1]]
        steady = [t for k, t in enumerate(t_obs) if k and k not in grew] or t_obs
        emit('voxel %g m: %d observe calls of %d rays: %s (calls without a growth of the tables, the first left out: %s); V per call median %d, min %d, max %d; '
             'cuts for the visit budget per call median %d, max %d; rays walked %d, dropped %d, skipped %d, truncated %d, visits %d (%.1f per walked ray); '
             'table %d .. %d voxels (capacity %d, grown in calls %s); see_through on the same rays, same session, map of 0 .. %d voxels: %s'
             % (vs, len(t_obs), n, stats(t_obs), stats(steady), int(np.median(visits)), min(visits), max(visits), int(np.median(splits)), max(splits),
                c['walked'], c['dropped'], c['skipped'], c['truncated'], c['visits'], c['visits'] / max(c['walked'], 1), sizes[0], sizes[-1], sp.capacity,
                grew, cloud.num_voxels, stats(t_see[1:])))
        q = max(1, len(t_obs) // 4)
        for lo in range(0, len(t_obs), q):
            hi = min(lo + q, len(t_obs))
            emit('  windows %2d-%2d: table -> %9d voxels, observe median %.2f ms (max %.2f), V median %d, see_through median %.2f ms'
                 % (lo, hi - 1, sizes[hi - 1], float(np.median(t_obs[lo:hi])), max(t_obs[lo:hi]), int(np.median(visits[lo:hi])), float(np.median(t_see[lo:hi]))))
        pts, _, T = windows[-1]
        t_look = [timed(lambda: sp.lookup(pts, T))[0] for _ in range(a.repeats)]
        res = sp.lookup(pts, T)
        emit('  lookup of %d points in the table of %d voxels: %s; counters rows, valid, seen, enough = %s'
             % (n, sp.num_voxels, stats(t_look[1:] or t_look), res['counters'].tolist()))
        del cloud, sp
        torch.cuda.synchronize()
    emit('not measured: the split of a call between the two walks, the sort and the merge; achieved bandwidth; any counter run')


if __name__ == '__main__':
    main()
