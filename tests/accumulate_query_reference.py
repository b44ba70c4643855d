"""Plain-Python restatement of the query contract of the accumulated scene cloud (include/pcacc.h C9), the reference of tests/test_accumulate_query.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]) and a {coord: rays} dict.  The own
voxel is a dict lookup of the point's voxel coordinates; the nearest kept centroid loops the 27 offsets in ascending (x, y, z) over a dict of
coordinates.  No key is formed and no row is searched, so a key whose field overflowed cannot alias another voxel here by accident.  All arithmetic is
Python floats (IEEE float64, never contracted) in the literal order of the contract; np.float32 only for `nearest` and for widening the inputs.
The float32 normals and their flags are an INPUT (C5 has its own tests): the rows of normals() under the same filter, or None."""
import math

import numpy as np

import accumulate_prune_reference as rref

INVALID, OCCUPIED, KEPT, MATCHED, NORMAL = 1, 2, 4, 8, 16
BIAS, LIMIT = 1 << 20, 32768.0
FIELDS = ('status', 'count', 'moving', 't_first', 't_last', 'pierced', 'row', 'nearest', 'distance', 'plane_distance')
DTYPES = dict(status=np.uint8, count=np.int64, moving=np.int64, t_first=np.int32, t_last=np.int32, pierced=np.int32, row=np.int32, nearest=np.float32,
              distance=np.float64, plane_distance=np.float64)
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]


def world(T, p, voxel_size):
    """-> (w [3] floats, idx [3] ints) or None for an invalid point."""
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    w, idx = [], []
    for a in range(3):
        v = ((T[a][0] * x + T[a][1] * y) + T[a][2] * z) + T[a][3]
        if math.isnan(v) or math.isinf(v) or not abs(v) < LIMIT:
            return None
        c = math.floor(v / voxel_size)
        if not -BIAS <= c < BIAS:
            return None
        w.append(v)
        idx.append(int(c))
    return w, idx


def kept_voxels(rmap, min_count=1, max_moving_fraction=None):
    """[(coord, centroid [3] floats)] of the voxels the filter keeps, in ascending (x, y, z): position = extract's row."""
    out = []
    for key, r in rmap.rec.items():
        if rref.keep(r[0], r[1], min_count, max_moving_fraction):
            out.append((rref.coord_of(key), [(float(r[2 + a]) / float(r[0])) * (1.0 / 65536.0) for a in range(3)]))
    out.sort(key=lambda t: t[0])
    return out


def query(rmap, pierced, points, pose=None, max_distance=None, min_count=1, max_moving_fraction=None, normals32=None, flags=None, require_normal=False,
          bad_table=False):
    """-> dict of numpy columns (FIELDS) and 'counters' (a list of 7).  bad_table: the normal tables do not have the rows the filter keeps."""
    vs = float(rmap.voxel_size)
    max_distance = vs if max_distance is None else float(max_distance)
    max_d2 = max_distance * max_distance
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))[:3]]
    own = {rref.coord_of(key): r for key, r in rmap.rec.items()}
    kept = kept_voxels(rmap, min_count, max_moving_fraction)
    where = {c: j for j, (c, _) in enumerate(kept)}
    have_normals = normals32 is not None and len(kept) > 0
    if have_normals and not bad_table:
        assert normals32.shape == (len(kept), 3) and flags.shape == (len(kept),)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = points.shape[0]
    out = {f: np.zeros((n, 3) if f == 'nearest' else (n,), DTYPES[f]) for f in FIELDS}
    out['row'][:] = -1
    out['distance'][:] = np.inf
    out['plane_distance'][:] = np.inf
    for i in range(n):
        wi = world(T, points[i], vs)
        if wi is None:
            out['status'][i] = INVALID
            continue
        w, idx = wi
        status = 0
        r = own.get(tuple(idx))
        if r is not None:
            status |= OCCUPIED
            out['count'][i], out['moving'][i], out['t_first'][i], out['t_last'][i] = r[0], r[1], r[5], r[6]
            out['pierced'][i] = 0 if pierced is None else pierced.get(tuple(idx), 0)
            if rref.keep(r[0], r[1], min_count, max_moving_fraction):
                status |= KEPT
        best, best_d2, best_e = -1, 0.0, None
        if not (have_normals and bad_table):
            for dx, dy, dz in OFFSETS:
                c = (idx[0] + dx, idx[1] + dy, idx[2] + dz)
                if not all(-BIAS <= v < BIAS for v in c):
                    continue
                j = where.get(c)
                if j is None:
                    continue
                if require_normal and have_normals and int(flags[j]) & 3:
                    continue
                cen = kept[j][1]
                ex, ey, ez = w[0] - cen[0], w[1] - cen[1], w[2] - cen[2]
                d2 = (ex * ex + ey * ey) + ez * ez
                if best < 0 or d2 < best_d2:
                    best, best_d2, best_e = j, d2, (ex, ey, ez)
        if best >= 0 and best_d2 <= max_d2:
            status |= MATCHED
            out['row'][i] = best
            out['nearest'][i] = np.array(kept[best][1], np.float64).astype(np.float32)
            out['distance'][i] = math.sqrt(best_d2)
            if have_normals and not int(flags[best]) & 3:
                nx, ny, nz = (float(v) for v in normals32[best])
                out['plane_distance'][i] = (nx * best_e[0] + ny * best_e[1]) + nz * best_e[2]
                status |= NORMAL
        out['status'][i] = status
    s = out['status']
    out['counters'] = [n] + [int(((s & bit) != 0).sum()) for bit in (INVALID, OCCUPIED, KEPT, MATCHED, NORMAL)] + [1 if (have_normals and bad_table and n > 0) else 0]
    return out


def brute_force(rmap, points, pose=None, max_distance=None, min_count=1, max_moving_fraction=None):
    """The global nearest kept centroid of every point, over ALL kept float64 centroids (ties to the lowest key = the first row), accepted within
    max_distance: -> (valid [n] bool, row [n] (-1 = none), distance [n] (+inf = none)).  The same d2 formula, vectorised over the rows."""
    vs = float(rmap.voxel_size)
    max_distance = vs if max_distance is None else float(max_distance)
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))[:3]]
    cen = np.array([c for _, c in kept_voxels(rmap, min_count, max_moving_fraction)], np.float64).reshape(-1, 3)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = points.shape[0]
    valid, row, dist = np.zeros(n, bool), np.full(n, -1, np.int64), np.full(n, np.inf)
    for i in range(n):
        wi = world(T, points[i], vs)
        if wi is None or cen.shape[0] == 0:
            valid[i] = wi is not None
            continue
        valid[i] = True
        e = np.array(wi[0], np.float64)[None, :] - cen
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        j = int(np.argmin(d2))                                                     # the first minimum: the lowest key
        if d2[j] <= max_distance * max_distance:
            row[i], dist[i] = j, math.sqrt(float(d2[j]))
    return valid, row, dist
