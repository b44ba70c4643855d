"""Time the merge and the regrid of observed space (include/pcacc.h C15, ObservedSpace.merge / regrid) on the 40-window drifting scene of
tools/bench_accumulate.py (5 x 160 k points per window, the sensor 1.8 m above the window's origin): space A observes windows 0 .. 19, space B windows
20 .. 39, then
  A.merge(B);  B.regrid(pose) at the same voxel size;  B.regrid(pose, 2 x voxel);  A.merge(B, pose)
each on a fresh copy of A, device events around the call (its one read-back of the counters included), one warm-up, --repeats times.  Beside each, in
the same session, the only route there was before: records() of the tables to the host, a numpy join there (the same arithmetic, float64, in the
contract's order), and the columns written back to device tables -- a host clock around it, ending in a device synchronise.  The two results are
asserted equal, column for column.
The windows of this scene are INDEPENDENT random clouds: the figures give sizes and memory behaviour.  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_accumulate_observe_merge.py [--windows 40] [--voxel 0.1] [--out profiles/accum_observe_merge_bench.txt]"""
import time

import numpy as np

from accum_bench import BIAS, SENSOR, Report, header, parser, scene, stats, timed, voxel_coords


def session_pose():
    """B's frame to A's: 30 degrees about z and a translation."""
    T = np.eye(4)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = (0.37, -0.21, 0.04)
    return T


def host_merge(a, b):
    """The numpy join of two tables (keys, rays, stamps [2,m]), both ascending and duplicate-free -> the union's columns."""
    (ka, ra, sa), (kb, rb, sb) = a, b
    keys = np.union1d(ka, kb)
    ia, ib = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    rays = np.zeros(keys.shape[0], np.int64)
    rays[ia] += ra
    rays[ib] += rb
    first = np.full(keys.shape[0], np.iinfo(np.int32).max, np.int32)
    last = np.full(keys.shape[0], np.iinfo(np.int32).min, np.int32)
    first[ia] = sa[0]
    last[ia] = sa[1]
    first[ib] = np.minimum(first[ib], sb[0])
    last[ib] = np.maximum(last[ib], sb[1])
    return keys, rays, np.stack([first, last])


def host_regrid(table, pose, in_voxel_size, out_voxel_size):
    """The numpy regrid of a table: centres under the pose (float64, ((a + b) + c) + d), floor division by out_voxel_size, rows of one key folded to the
    maximum ray count, the minimum first and the maximum last stamp -> (the columns, rows dropped)."""
    keys, rays, stamps = table
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    c = np.stack(voxel_coords(keys), 1)
    p = (c.astype(np.float64) + 0.5) * np.float64(in_voxel_size)
    valid = np.ones(keys.shape[0], bool)
    out_key = np.zeros(keys.shape[0], np.int64)
    with np.errstate(all='ignore'):
        for a, shift in enumerate((42, 21, 0)):
            w = ((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3]
            i = np.floor(w / np.float64(out_voxel_size))
            ok = np.isfinite(w) & (np.abs(w) < 32768.0) & (i >= -float(BIAS)) & (i < float(BIAS))
            valid &= ok
            out_key |= (np.where(ok, i, 0).astype(np.int64) + BIAS) << shift
    order = np.argsort(out_key[valid], kind='stable')
    k, r, s0, s1 = out_key[valid][order], rays[valid][order], stamps[0][valid][order], stamps[1][valid][order]
    if k.shape[0] == 0:
        return (k, r, np.stack([s0, s1])), int((~valid).sum())
    heads = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    return (k[heads], np.maximum.reduceat(r, heads), np.stack([np.minimum.reduceat(s0, heads), np.maximum.reduceat(s1, heads)])), int((~valid).sum())


def parse_args(argv=None):
    ap = parser('accum_observe_merge_bench.txt', repeats=5, baseline=False)
    ap.add_argument('--max-steps', type=int, default=4096)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd.accumulate import ObservedSpace
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--max-steps %d --repeats %d' % (a.max_steps, a.repeats),
                                'device events around each call, one warm-up; the host route by a host clock that ends in a synchronise')).emit
    half = a.windows // 2
    spaces = [ObservedSpace(a.voxel, dev), ObservedSpace(a.voxel, dev)]
    for k, pts, moving, T in scene(a, dev):
        spaces[k >= half].observe(pts, SENSOR, pose=T, moving=moving, stamp=k, max_steps=a.max_steps)
        if k % 10 == 9:
            print('scene: %d windows observed' % (k + 1), flush=True)
    A, B = spaces
    del pts, moving
    pose = session_pose()
    emit('space A: windows 0 .. %d, %d voxels (capacity %d); space B: windows %d .. %d, %d voxels (capacity %d); voxel %g m'
         % (half - 1, A.num_voxels, A.capacity, half, a.windows - 1, B.num_voxels, B.capacity, a.voxel))

    def to_device(table):
        out = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in table)
        torch.cuda.synchronize()
        return out

    def host_route(fn):
        t0 = time.perf_counter()
        out = to_device(fn())
        return (time.perf_counter() - t0) * 1e3, out

    def same(space, table, what):
        keys, rays, stamps = space._cur
        n = space.num_voxels
        assert n == table[0].shape[0], (what, n, table[0].shape[0])
        assert torch.equal(keys[:n], table[0]) and torch.equal(rays[:n], table[1]) and torch.equal(stamps[:, :n], table[2]), what

    warm = A.copy()                                                              # warm-up: code objects, allocator, the sort's first call
    warm.merge(B, pose=pose)
    B.regrid(voxel_size=2 * a.voxel)
    del warm

    jobs = (('A.merge(B)', lambda c: c.merge(B), lambda: host_merge(A.records(), B.records()), True),
            ('B.regrid(pose), voxel %g m' % a.voxel, lambda c: B.regrid(pose), lambda: host_regrid(B.records(), pose, a.voxel, a.voxel)[0], False),
            ('B.regrid(pose, voxel %g m)' % (2 * a.voxel), lambda c: B.regrid(pose, 2 * a.voxel),
             lambda: host_regrid(B.records(), pose, a.voxel, 2 * a.voxel)[0], False),
            ('A.merge(B, pose)', lambda c: c.merge(B, pose=pose),
             lambda: host_merge(A.records(), host_regrid(B.records(), pose, a.voxel, a.voxel)[0]), True))
    for name, device_fn, host_fn, into_copy in jobs:
        times, out = [], None
        for _ in range(a.repeats):
            c = A.copy() if into_copy else None
            if into_copy:
                c._alt = tuple(torch.empty_like(t) for t in c._cur)              # the second set of tables, as a space that has observed holds it
            torch.cuda.synchronize()
            t, res = timed(lambda: device_fn(c))
            times.append(t)
            out = c if into_copy else res
            del c, res
        host_ms, table = host_route(host_fn)
        same(out, table, name)
        info = ('%d rows' % out.num_voxels) + ('' if into_copy else ', %d dropped' % out.dropped_rows)
        emit('%s: %s -> %s; host route (records, numpy, write back), once: %.0f ms; results equal' % (name, stats(times), info, host_ms))
        del out, table
    emit('not measured: achieved bandwidth; the split of a call between search, sort and write; other scenes; any counter run')


if __name__ == '__main__':
    main()
