"""Plain-Python restatement of the ray-cast contract of the accumulated scene cloud (include/pcacc.h C10), the reference of
tests/test_accumulate_raycast.py.

The map is a dict of voxel coordinates, (x, y, z) -> (extract's row, float64 centroid), of the voxels the filter keeps.  Python floats are IEEE float64
and Python never contracts a product and a sum, so writing the contract's operations down in its literal order gives its bits.  No key is formed and no
row is searched: a visit is a dict lookup.  np.float32 only for `point` and for widening the inputs."""
import math

import numpy as np

import accumulate_query_reference as qref

MISS, HIT, TRUNCATED, SKIPPED, DROPPED = range(5)
BIAS, LIMIT = 1 << 20, 32768.0
FIELDS = ('status', 'row', 'coords', 'point', 'range_in', 'depth', 'length', 'visits')
DTYPES = dict(status=np.uint8, row=np.int32, coords=np.int32, point=np.float32, range_in=np.float64, depth=np.float64, length=np.float64, visits=np.int32)
WIDE = ('coords', 'point')


def kept_dict(rmap, min_count=1, max_moving_fraction=None):
    """{coord: (row of extract, centroid [3] floats)} of the voxels the filter keeps."""
    return {c: (j, cen) for j, (c, cen) in enumerate(qref.kept_voxels(rmap, min_count, max_moving_fraction))}


def end_point(T, x, y, z, vs):
    """-> (w, idx) or None when C4's validity rule fails."""
    w, idx = [], []
    for a in range(3):
        v = ((T[a][0] * x + T[a][1] * y) + T[a][2] * z) + T[a][3]
        if math.isnan(v) or math.isinf(v) or not abs(v) < LIMIT:
            return None
        c = v / vs
        if math.isnan(c) or math.isinf(c):
            return None
        c = math.floor(c)
        if not -BIAS <= c < BIAS:
            return None
        w.append(v)
        idx.append(int(c))
    return w, idx


def ray(kept, T, p, origin, vs, min_range, max_range, margin, max_steps):
    """One ray -> dict(status, row, coords, centroid, range_in, depth, length, visits, visited, geom): visited = [(coord, t_in)] in walking order,
    geom = (o, d, L, t_start, t_end) of a walked ray."""
    res = dict(status=DROPPED, row=-1, coords=(0, 0, 0), centroid=None, range_in=math.inf, depth=math.inf, length=0.0, visits=0, visited=[], geom=None)
    if origin is None:
        return res
    o = end_point(T, float(origin[0]), float(origin[1]), float(origin[2]), vs)
    if o is None:
        return res
    e = end_point(T, float(p[0]), float(p[1]), float(p[2]), vs)
    if e is None:
        return res
    res['status'] = SKIPPED
    o, i = o[0], list(o[1])
    e = e[0]
    d = [e[0] - o[0], e[1] - o[1], e[2] - o[2]]
    L = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    res['length'] = L
    if not L > 0.0:
        return res
    t_start = min_range / L
    t_end = max_range / L if max_range is not None else 1.0 - margin / L
    if not t_end > 0.0 or not t_start < t_end:
        return res
    res['status'] = MISS
    res['geom'] = (o, d, L, t_start, t_end)
    t_in = 0.0
    while True:
        res['visits'] += 1
        res['visited'].append((tuple(i), t_in))
        if not t_in < t_start:
            found = kept.get(tuple(i))
            if found is not None:
                c = found[1]
                res.update(status=HIT, row=found[0], coords=tuple(i), centroid=c, range_in=t_in * L,
                           depth=(((c[0] - o[0]) * d[0] + (c[1] - o[1]) * d[1]) + (c[2] - o[2]) * d[2]) / L)
                return res
        best, t_best = -1, 0.0
        for a in range(3):
            if d[a] == 0.0:
                continue
            b = float(i[a] + (1 if d[a] > 0.0 else 0)) * vs
            t = (b - o[a]) / d[a]
            if best < 0 or t < t_best:
                best, t_best = a, t
        if best < 0 or not t_best < t_end:
            return res
        i[best] += 1 if d[best] > 0.0 else -1
        if not -BIAS <= i[best] < BIAS:
            return res
        t_in = t_best
        if res['visits'] >= max_steps:
            res['status'] = TRUNCATED
            return res


def raycast(rmap, targets, origins, origin_index=None, pose=None, max_range=None, min_range=0.0, margin=0.0, min_count=1, max_moving_fraction=None,
            max_steps=4096, rays=None):
    """-> dict of numpy columns (FIELDS) and 'counters' (a list of 7).  rays: a list that receives every ray's dict."""
    vs = float(rmap.voxel_size)
    kept = kept_dict(rmap, min_count, max_moving_fraction)
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))[:3]]
    pts = np.asarray(targets, np.float32).reshape(-1, 3)
    org = np.asarray(origins, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    out = {f: np.zeros((n, 3) if f in WIDE else (n,), DTYPES[f]) for f in FIELDS}
    counters = [n, 0, 0, 0, 0, 0, 0]
    for k in range(n):
        row = 0 if origin_index is None else int(origin_index[k])
        r = ray(kept, T, pts[k], org[row] if 0 <= row < org.shape[0] else None, vs, float(min_range), None if max_range is None else float(max_range),
                float(margin), int(max_steps))
        if rays is not None:
            rays.append(r)
        out['status'][k], out['row'][k], out['coords'][k] = r['status'], r['row'], r['coords']
        if r['centroid'] is not None:
            out['point'][k] = np.array(r['centroid'], np.float64).astype(np.float32)
        out['range_in'][k], out['depth'][k], out['length'][k], out['visits'][k] = r['range_in'], r['depth'], r['length'], r['visits']
        counters[{DROPPED: 1, SKIPPED: 2, HIT: 3, MISS: 4, TRUNCATED: 5}[r['status']]] += 1
        counters[6] += r['visits']
    out['counters'] = counters
    return out
