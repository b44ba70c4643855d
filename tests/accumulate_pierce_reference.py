"""Plain-Python restatement of the ray contract of the accumulated scene cloud (include/pcacc.h C7), the reference of tests/test_accumulate_pierce.py.

The map is a dict of voxel coordinates, (x, y, z) -> (t_first, t_last); the counts are a dict of coordinates too.  Python floats are IEEE float64 and
Python never contracts a product and a sum, so writing the contract's operations down in its literal order gives its bits.  No key is formed and no
row is searched: a visit is a dict lookup."""
import math

import numpy as np

BIAS = 1 << 20
LIMIT = 32768.0
WALKED, DROPPED, SKIPPED, TRUNCATED, HITS = range(5)


def voxels_of(ref_map):
    """{(x, y, z): (t_first, t_last)} of an accumulate_reference.ReferenceMap."""
    out = {}
    for key, r in ref_map.rec.items():
        out[((key >> 42) - BIAS, ((key >> 21) & 0x1fffff) - BIAS, (key & 0x1fffff) - BIAS)] = (r[5], r[6])
    return out


def _end_point(T, x, y, z, vs):
    """-> (w, idx) or None when C4's validity rule fails."""
    w, idx = [], []
    for a in range(3):
        v = ((T[a][0] * x + T[a][1] * y) + T[a][2] * z) + T[a][3]
        if not math.isfinite(v) or not abs(v) < LIMIT:
            return None
        c = v / vs
        if not math.isfinite(c):
            return None
        c = math.floor(c)
        if not -BIAS <= c < BIAS:
            return None
        w.append(v)
        idx.append(c)
    return w, idx


def ray(T, p, origin, moving, vs, margin, max_range, max_steps):
    """One ray -> (status, truncated, visited): visited = the list of voxel coordinates in walking order, t_end as its fourth entry for WALKED."""
    if origin is None:
        return DROPPED, False, [], None
    o = _end_point(T, float(origin[0]), float(origin[1]), float(origin[2]), vs)
    if o is None:
        return DROPPED, False, [], None
    e = _end_point(T, float(p[0]), float(p[1]), float(p[2]), vs)
    if e is None:
        return DROPPED, False, [], None
    if moving:
        return SKIPPED, False, [], None
    o, i = o[0], list(o[1])
    e = e[0]
    d = [e[0] - o[0], e[1] - o[1], e[2] - o[2]]
    L = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if not L > 0.0:
        return SKIPPED, False, [], None
    t_end = 1.0 - margin / L
    if max_range is not None:
        t_end = min(t_end, max_range / L)
    if not t_end > 0.0:
        return SKIPPED, False, [], None
    visited, truncated = [], False
    while True:
        visited.append(tuple(i))
        best, t_best = -1, 0.0
        for a in range(3):
            if d[a] == 0.0:
                continue
            b = float(i[a] + (1 if d[a] > 0.0 else 0)) * vs
            t = (b - o[a]) / d[a]
            if best < 0 or t < t_best:
                best, t_best = a, t
        if best < 0 or not t_best < t_end:
            break
        i[best] += 1 if d[best] > 0.0 else -1
        if not -BIAS <= i[best] < BIAS:
            break
        if len(visited) >= max_steps:
            truncated = True
            break
    return WALKED, truncated, visited, (o, d, L, t_end)


def pierce(voxels, points, origins, origin_index=None, pose=None, moving=None, voxel_size=0.1, margin=None, max_range=None, stamp=None, max_steps=4096,
           pierced=None, counters=None, walks=None):
    """The rays of one call.  voxels: {coord: (t_first, t_last)}; points [n,3] float32; origins [S,3] float64.  Adds to `pierced` ({coord: count}, only
    voxels of the map appear) and to `counters` (5 integers) and returns both.  walks: a list that receives (ray number, visited, (o, d, L, t_end)) of
    every walked ray."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    org = np.asarray(origins, np.float64).reshape(-1, 3)
    T = [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))]
    vs = float(voxel_size)
    margin = 2.0 * vs if margin is None else float(margin)
    pierced = {} if pierced is None else pierced
    counters = [0] * 5 if counters is None else counters
    for n in range(pts.shape[0]):
        row = 0 if origin_index is None else int(origin_index[n])
        origin = org[row] if 0 <= row < org.shape[0] else None
        status, truncated, visited, geom = ray(T, pts[n], origin, moving is not None and bool(moving[n]), vs, margin,
                                              None if max_range is None else float(max_range), max_steps)
        counters[status] += 1
        counters[TRUNCATED] += int(truncated)
        if walks is not None and status == WALKED:
            walks.append((n, visited, geom))
        for c in visited:
            t = voxels.get(c)
            if t is not None and (stamp is None or t[1] < stamp or t[0] > stamp):
                pierced[c] = pierced.get(c, 0) + 1
                counters[HITS] += 1
    return pierced, counters


def aligned(pierced, coords):
    """The dict's counts in the row order of `coords` [V,3]: int32 [V]."""
    return np.array([pierced.get(tuple(c), 0) for c in np.asarray(coords).reshape(-1, 3).tolist()], np.int32)
