"""numpy restatement of the accumulated scene cloud's contract (include/pcacc.h C4), the reference of tests/test_accumulate.py.

Element-wise float64 in the literal operation order of the contract (no `@`: BLAS may fuse), np.floor, np.rint, np.unique over the keys, int64 sums,
and the extract formula.  The claim against it is equality: identical integer records, bit-identical float32 centroids."""
import numpy as np

BIAS = 1 << 20
LIMIT = 32768.0
FIXED = 65536.0


def per_point(points, pose, voxel_size):
    """-> valid [n] bool, key [n] int64 (0 where invalid), q [n,3] int64 (0 where invalid)."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    vs = np.float64(voxel_size)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    valid = np.ones(p.shape[0], bool)
    idx, q = [], []
    with np.errstate(all='ignore'):
        for a in range(3):
            w = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
            i = np.floor(w / vs)
            ok = np.isfinite(w) & (np.abs(w) < LIMIT)
            ok &= (i >= -BIAS) & (i < BIAS)
            valid &= ok
            idx.append(np.where(ok, i, 0.0).astype(np.int64))
            q.append(np.where(ok, np.rint(w * FIXED), 0.0).astype(np.int64))
    key = ((idx[0] + BIAS) << 42) | ((idx[1] + BIAS) << 21) | (idx[2] + BIAS)
    return valid, np.where(valid, key, 0), np.where(valid[:, None], np.stack(q, 1), 0)


class ReferenceMap(object):
    """The map as a dict: key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last] of Python integers."""

    def __init__(self, voxel_size):
        self.voxel_size = float(voxel_size)
        self.rec = {}
        self.dropped = 0

    def add(self, points, pose=None, moving=None, stamp=0):
        points = np.asarray(points, np.float32).reshape(-1, 3)
        n = points.shape[0]
        valid, key, q = per_point(points, pose, self.voxel_size)
        mv = np.zeros(n, np.int64) if moving is None else (np.asarray(moving) != 0).astype(np.int64)
        self.dropped += int(n - valid.sum())
        key, q, mv = key[valid], q[valid], mv[valid]
        uniq, inv = np.unique(key, return_inverse=True)
        sums = np.zeros((uniq.shape[0], 5), np.int64)
        np.add.at(sums, inv, np.concatenate([np.ones((key.shape[0], 1), np.int64), mv[:, None], q], 1))
        for k, s in zip(uniq.tolist(), sums.tolist()):
            r = self.rec.get(k)
            if r is None:
                self.rec[k] = s + [int(stamp), int(stamp)]
            else:
                self.rec[k] = [r[f] + s[f] for f in range(5)] + [min(r[5], int(stamp)), max(r[6], int(stamp))]
        return self

    def add_loop(self, points, pose=None, moving=None, stamp=0):
        """The same as add, point by point in plain Python (the self-check of the np.unique formulation)."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        valid, key, q = per_point(points, pose, self.voxel_size)
        for i in range(points.shape[0]):
            if not valid[i]:
                self.dropped += 1
                continue
            m = 0 if moving is None else int(moving[i] != 0)
            r = self.rec.setdefault(int(key[i]), [0, 0, 0, 0, 0, int(stamp), int(stamp)])
            r[0] += 1
            r[1] += m
            for a in range(3):
                r[2 + a] += int(q[i, a])
            r[5], r[6] = min(r[5], int(stamp)), max(r[6], int(stamp))
        return self

    @property
    def num_voxels(self):
        return len(self.rec)

    def records(self):
        """keys [M] i64 ascending, acc [5,M] i64, stamps [2,M] i32 -- the layout AccumulatedCloud.records() returns."""
        keys = np.array(sorted(self.rec), np.int64)
        rows = np.array([self.rec[k] for k in keys.tolist()], np.int64).reshape(-1, 7)
        return keys, np.ascontiguousarray(rows[:, :5].T), np.ascontiguousarray(rows[:, 5:].T).astype(np.int32)

    def extract(self, min_count=1, max_moving_fraction=None):
        keys, acc, stamps = self.records()
        count, moving = acc[0], acc[1]
        keep = count >= min_count
        if max_moving_fraction is not None:
            keep &= moving.astype(np.float64) / count.astype(np.float64) <= np.float64(max_moving_fraction)
        keys, acc, stamps = keys[keep], acc[:, keep], stamps[:, keep]
        pts = ((acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * np.float64(2.0 ** -16)).astype(np.float32)
        coords = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - BIAS
        return {'points': pts.reshape(-1, 3), 'coords': coords.astype(np.int32).reshape(-1, 3), 'count': acc[0], 'moving': acc[1],
                't_first': stamps[0], 't_last': stamps[1]}
