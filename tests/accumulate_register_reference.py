"""numpy restatement of the scan-to-map registration of the accumulated scene cloud (include/pcacc.h C6), the reference of
tests/test_accumulate_register.py, on top of accumulate_reference.ReferenceMap.

A dict from voxel coordinates to row (no keys), the 27 offsets in ascending (x, y, z) order, float64 everywhere, numpy's own sums (pairwise, not the
header's slots) and np.linalg.solve instead of the scaled Cholesky; the update rule and the round logic are the contract's.  The float32 normals and
their flags are an INPUT (C5 has its own tests).  Against the header the claim is equality for integers (rows, counts, status, iterations) and a
bound for pose, fitness and rmse: the two differ only in summation order and in the solver."""
import numpy as np

import accumulate_normals_reference as nref
import accumulate_reference as ref

NO_ELIGIBLE, NO_CANDIDATE, NO_CORRESPONDENCE, DEGENERATE, MAX_ITER, BAD_TABLE = 1, 2, 4, 8, 16, 32
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]


def world(points, T, voxel_size):
    """-> w [n,3] f64, idx [n,3] i64, valid [n]: the literal operation order of C4's transform."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    valid = np.ones(p.shape[0], bool)
    w, idx = [], []
    with np.errstate(all='ignore'):
        for a in range(3):
            v = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
            i = np.floor(v / np.float64(voxel_size))
            ok = np.isfinite(v) & (np.abs(v) < ref.LIMIT) & (i >= -ref.BIAS) & (i < ref.BIAS)
            valid &= ok
            w.append(np.where(ok, v, 0.0))
            idx.append(np.where(ok, i, 0.0).astype(np.int64))
    return np.stack(w, 1).reshape(-1, 3), np.stack(idx, 1).reshape(-1, 3), valid


def compose(x, T):
    h = x[:3] / 2.0
    q = np.concatenate([[1.0], h]) / np.sqrt(1.0 + h @ h)
    qw, qx, qy, qz = q
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                  [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                  [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = R, x[3:]
    return D @ T


def register(rmap, normals32, flags, points, init_pose=None, moving=None, max_distance=None, max_iter=30, min_count=1, max_moving_fraction=None):
    """normals32 [V,3] f32 / flags [V] u8: the rows of normals() under (min_count, max_moving_fraction).  -> dict: pose [4,4], fitness, rmse,
    iterations, status, correspondences, first / last [n] (the matched MAP row of every point in the first / last evaluation, -1 = none)."""
    keys_all = rmap.records()[0]
    keys, acc, _ = nref.kept_records(rmap, min_count, max_moving_fraction)
    map_row = np.flatnonzero(np.isin(keys_all, keys))
    v = keys.shape[0]
    assert normals32.shape == (v, 3) and flags.shape == (v,)
    coords = (np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - ref.BIAS).reshape(v, 3)
    cent = ((acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * np.float64(2.0 ** -16)).reshape(v, 3)
    ok_row = (flags & 3) == 0
    where = {tuple(c): j for j, c in enumerate(coords.tolist()) if ok_row[j]}
    nrm = normals32.astype(np.float64)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = points.shape[0]
    mv = np.zeros(n, bool) if moving is None else np.asarray(moving) != 0
    eligible = int((~mv).sum())
    max_distance = rmap.voxel_size if max_distance is None else max_distance
    T = np.eye(4) if init_pose is None else np.array(init_pose, np.float64)
    T[3] = (0, 0, 0, 1)
    T_good = T.copy()
    out = {'first': np.full(n, -1, np.int64), 'last': np.full(n, -1, np.int64)}

    def finish(pose, fit, rmse, iters, status, nc):
        out.update(pose=pose.copy(), fitness=fit, rmse=rmse, iterations=iters, status=status, correspondences=int(nc))
        return out

    prev_fit = prev_rmse = 0.0
    iters = 0
    for rnd in range(max_iter + 1):
        w, idx, valid = world(points, T, rmap.voxel_size)
        use = valid & ~mv
        d2 = np.full((n, 27), np.inf)
        rows = np.full((n, 27), -1, np.int64)
        if where:
            for o, (dx, dy, dz) in enumerate(OFFSETS):
                c = idx + (dx, dy, dz)
                inside = use & np.all((c >= -ref.BIAS) & (c < ref.BIAS), 1)
                j = np.array([where.get(t, -1) for t in map(tuple, c.tolist())], np.int64).reshape(n)
                j[~inside] = -1
                hit = j >= 0
                e = w[hit] - cent[j[hit]]
                d2[hit, o] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                rows[hit, o] = j[hit]
        best = np.argmin(d2, 1) if n else np.zeros(0, np.int64)                   # the first minimum: the lowest key
        bd2 = d2[np.arange(n), best]
        matched = bd2 <= np.float64(max_distance) * np.float64(max_distance)
        j = rows[np.arange(n), best][matched]
        now = np.full(n, -1, np.int64)
        now[matched] = map_row[j]
        if rnd == 0:
            out['first'] = now
        out['last'] = now
        if eligible == 0 or not where:
            return finish(T_good, 0.0, 0.0, iters, (NO_ELIGIBLE if eligible == 0 else 0) | (0 if where else NO_CANDIDATE), 0)
        nc = int(matched.sum())
        if nc == 0:
            return finish(T_good, 0.0, 0.0, iters, NO_CORRESPONDENCE, 0)
        wm, nm = w[matched], nrm[j]
        r = ((wm - cent[j]) * nm).sum(1)
        J = np.concatenate([np.cross(wm, nm), nm], 1)
        fit, rmse = nc / eligible, np.sqrt((r * r).sum() / nc)
        T_good = T.copy()
        converged = rnd > 0 and abs(fit - prev_fit) < 1e-6 and abs(rmse - prev_rmse) < 1e-6
        if converged or rnd >= max_iter:
            return finish(T, fit, rmse, rnd, 0 if converged else MAX_ITER, nc)
        A, b = J.T @ J, J.T @ r
        d = np.sqrt(np.diag(A))
        if np.any(d <= 0) or np.linalg.eigvalsh(A / np.outer(d, d)).min() <= 1e-10:
            return finish(T, 0.0, 0.0, rnd, DEGENERATE, nc)
        T = compose(np.linalg.solve(A, -b), T)
        prev_fit, prev_rmse, iters = fit, rmse, rnd + 1
    raise AssertionError('unreachable')
