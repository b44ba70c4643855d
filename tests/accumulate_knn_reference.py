"""Plain-Python restatement of the k-nearest contract of the accumulated scene cloud (include/pcacc.h C16), the reference of tests/test_accumulate_knn.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]).  The candidates of a query are
dict lookups of the (2r+1)^3 voxel coordinates around the query's voxel; the accepted ones are SORTED by (d2, row) and the first k taken.  No key is
formed, no row is searched and no running top-k is kept, so neither a key whose field overflowed nor the order of the visits can enter here by accident.
All arithmetic is Python floats (IEEE float64, never contracted) in the literal order of the contract; np.float32 only for widening the inputs.
world() and kept_voxels() are C9's (accumulate_query_reference.py)."""
import math

import numpy as np

import accumulate_query_reference as qref

INVALID, FOUND, FULL = 1, 2, 4
MAX_K, MAX_RADIUS = 16, 4
BIAS = qref.BIAS
FIELDS = ('rows', 'distance', 'found', 'status')
SELF_FIELDS = FIELDS + ('mean_distance',)
DTYPES = dict(rows=np.int32, distance=np.float64, found=np.int32, status=np.uint8, mean_distance=np.float64)


def _empty(n, k, self_mode):
    out = dict(rows=np.full((n, k), -1, np.int32), distance=np.full((n, k), np.inf), found=np.zeros(n, np.int32), status=np.zeros(n, np.uint8))
    if self_mode:
        out['mean_distance'] = np.full(n, np.inf)
    return out


def _neighbours(where, kept, w, idx, radius, max_d2, skip):
    """[(d2, row)] of the accepted candidates around voxel idx, sorted; skip = the row that is the query itself, or None."""
    got = []
    span = range(-radius, radius + 1)
    for dx in span:
        for dy in span:
            for dz in span:
                c = (idx[0] + dx, idx[1] + dy, idx[2] + dz)
                if not all(-BIAS <= v < BIAS for v in c):
                    continue
                j = where.get(c)
                if j is None or j == skip:
                    continue
                cen = kept[j][1]
                ex, ey, ez = w[0] - cen[0], w[1] - cen[1], w[2] - cen[2]
                d2 = (ex * ex + ey * ey) + ez * ez
                if d2 <= max_d2:
                    got.append((d2, j))
    got.sort()
    return got


def _fill(out, i, got, k):
    got = got[:k]
    total = 0.0
    for s, (d2, j) in enumerate(got):
        d = math.sqrt(d2)
        out['rows'][i, s], out['distance'][i, s] = j, d
        total = d if s == 0 else total + d
    out['found'][i] = len(got)
    out['status'][i] = (FOUND if got else 0) | (FULL if len(got) == k else 0)
    if 'mean_distance' in out and got:
        out['mean_distance'][i] = total / float(len(got))


def _counters(out):
    s, f = out['status'], out['found']
    return [len(s), int(((s & INVALID) != 0).sum()), int(((s & FOUND) != 0).sum()), int(((s & FULL) != 0).sum()), int(f.sum())]


def _args(rmap, radius, max_distance, min_count, max_moving_fraction):
    vs = float(rmap.voxel_size)
    max_distance = radius * vs if max_distance is None else float(max_distance)
    kept = qref.kept_voxels(rmap, min_count, max_moving_fraction)
    return vs, max_distance * max_distance, kept, {c: j for j, (c, _) in enumerate(kept)}


def knn(rmap, points, k, pose=None, radius=2, max_distance=None, min_count=1, max_moving_fraction=None):
    """Scan mode -> dict of numpy columns (FIELDS) and 'counters' (a list of 5)."""
    vs, max_d2, kept, where = _args(rmap, radius, max_distance, min_count, max_moving_fraction)
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))[:3]]
    points = np.asarray(points, np.float32).reshape(-1, 3)
    out = _empty(points.shape[0], k, False)
    for i in range(points.shape[0]):
        wi = qref.world(T, points[i], vs)
        if wi is None:
            out['status'][i] = INVALID
            continue
        _fill(out, i, _neighbours(where, kept, wi[0], wi[1], radius, max_d2, None), k)
    out['counters'] = _counters(out)
    return out


def neighbors(rmap, k, radius=2, max_distance=None, min_count=1, max_moving_fraction=None):
    """Self mode: one row per kept voxel, in extract's order -> dict of numpy columns (SELF_FIELDS) and 'counters'."""
    _, max_d2, kept, where = _args(rmap, radius, max_distance, min_count, max_moving_fraction)
    out = _empty(len(kept), k, True)
    for i, (coord, cen) in enumerate(kept):
        _fill(out, i, _neighbours(where, kept, cen, coord, radius, max_d2, i), k)
    out['counters'] = _counters(out)
    return out


def brute_force(rmap, k, queries, max_distance, min_count=1, max_moving_fraction=None, self_mode=False):
    """The k nearest kept centroids of every query over ALL kept float64 centroids, in (d2, row) order, accepted within max_distance.  queries: [n,3]
    float64 world points (scan mode), or None with self_mode (every kept centroid, itself excluded).  The same d2 formula, vectorised over the rows.
    -> rows [n,k] (-1 = none), distance [n,k] (+inf = none)."""
    cen = np.array([c for _, c in qref.kept_voxels(rmap, min_count, max_moving_fraction)], np.float64).reshape(-1, 3)
    queries = cen if self_mode else np.asarray(queries, np.float64).reshape(-1, 3)
    n = queries.shape[0]
    rows, dist = np.full((n, k), -1, np.int32), np.full((n, k), np.inf)
    for i in range(n):
        e = queries[i][None, :] - cen
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        ok = d2 <= max_distance * max_distance
        if self_mode:
            ok[i] = False
        order = [j for j in np.lexsort((np.arange(cen.shape[0]), d2)) if ok[j]][:k]
        rows[i, :len(order)] = order
        dist[i, :len(order)] = [math.sqrt(float(d2[j])) for j in order]
    return rows, dist


def world_points(points, voxel_size, pose=None):
    """The float64 world coordinates of the valid points of a scan and their mask, by C9's world()."""
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))[:3]]
    got = [qref.world(T, p, float(voxel_size)) for p in np.asarray(points, np.float32).reshape(-1, 3)]
    valid = np.array([g is not None for g in got], bool)
    return np.array([g[0] for g in got if g is not None], np.float64).reshape(-1, 3), valid


def outliers(rmap, k=8, std_ratio=2.0, **kw):
    """-> (mean_distance [V], threshold, mask [V]): threshold = mean + std_ratio * population std of the finite mean distances (numpy, float64)."""
    mean = neighbors(rmap, k, **kw)['mean_distance']
    finite = mean[np.isfinite(mean)]
    threshold = float(finite.mean() + std_ratio * finite.std()) if finite.size else float('nan')
    return mean, threshold, (mean > threshold) | ~np.isfinite(mean)

