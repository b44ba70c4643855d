"""Plain-Python restatement of the observed-space contract (include/pcacc.h C14), the reference of tests/test_accumulate_observe.py.

The table is a dict of voxel coordinates, (x, y, z) -> [rays, t_first, t_last], plus the five counters (walked, dropped, skipped, truncated, visits).
The walk of a ray is accumulate_pierce_reference.ray -- C7's restatement, Python floats in the contract's literal order.  No key is formed and nothing
is sorted: a visit is a dict update, a lookup a dict lookup."""
import math

import numpy as np

import accumulate_pierce_reference as pref

BIAS = pref.BIAS
WALKED, DROPPED, SKIPPED, TRUNCATED, VISITS = range(5)
VALID, SEEN, ENOUGH = 1, 2, 4
UNKNOWN, FREE, OCCUPIED = 0, 1, 2


def _pose(pose):
    return [[float(v) for v in row] for row in (np.eye(4) if pose is None else np.asarray(pose, np.float64))]


class ReferenceSpace(object):
    def __init__(self, voxel_size):
        self.voxel_size = float(voxel_size)
        self.rec = {}
        self.counters = [0] * 5

    def observe(self, points, origins, origin_index=None, pose=None, moving=None, stamp=0, margin=None, max_range=None, max_steps=4096, per_ray=None):
        """The rays of one call.  points [n,3] float32; origins [S,3] float64.  per_ray: a list that receives the visit count of every ray."""
        pts = np.asarray(points, np.float32).reshape(-1, 3)
        org = np.asarray(origins, np.float64).reshape(-1, 3)
        T = _pose(pose)
        vs = self.voxel_size
        margin = 2.0 * vs if margin is None else float(margin)
        for n in range(pts.shape[0]):
            row = 0 if origin_index is None else int(origin_index[n])
            origin = org[row] if 0 <= row < org.shape[0] else None
            status, truncated, visited, _ = pref.ray(T, pts[n], origin, moving is not None and bool(moving[n]), vs, margin,
                                                     None if max_range is None else float(max_range), max_steps)
            self.counters[status] += 1
            self.counters[TRUNCATED] += int(truncated)
            self.counters[VISITS] += len(visited)
            if per_ray is not None:
                per_ray.append(len(visited))
            for c in visited:
                r = self.rec.get(c)
                if r is None:
                    self.rec[c] = [1, stamp, stamp]
                else:
                    r[0] += 1
                    r[1] = min(r[1], stamp)
                    r[2] = max(r[2], stamp)
        return self

    def copy(self):
        c = ReferenceSpace(self.voxel_size)
        c.rec = {k: list(v) for k, v in self.rec.items()}
        c.counters = list(self.counters)
        return c

    def _row(self, coord, min_rays):
        """(status, rays, t_first, t_last) of a valid voxel."""
        r = self.rec.get(coord)
        if r is None:
            return VALID, 0, 0, 0
        return VALID | SEEN | (ENOUGH if r[0] >= min_rays else 0), r[0], r[1], r[2]

    def lookup(self, points, pose=None, min_rays=1):
        """-> [(status, rays, t_first, t_last)] per point: C4's transform and validity rule, then the voxel's row."""
        T = _pose(pose)
        out = []
        for p in np.asarray(points, np.float32).reshape(-1, 3):
            e = pref._end_point(T, float(p[0]), float(p[1]), float(p[2]), self.voxel_size)
            out.append((0, 0, 0, 0) if e is None else self._row(tuple(e[1]), min_rays))
        return out

    def lookup_voxels(self, coords, min_rays=1):
        out = []
        for c in np.asarray(coords, np.int64).reshape(-1, 3).tolist():
            out.append(self._row(tuple(c), min_rays) if all(-BIAS <= v < BIAS for v in c) else (0, 0, 0, 0))
        return out

    def occupancy(self, occupied, coords, min_rays=1):
        """occupied: the set of coordinates the cloud's extract holds -> [state] per row."""
        out = []
        for c in np.asarray(coords, np.int64).reshape(-1, 3).tolist():
            c = tuple(c)
            if not all(-BIAS <= v < BIAS for v in c):
                out.append(UNKNOWN)
            elif c in occupied:
                out.append(OCCUPIED)
            else:
                out.append(FREE if self._row(c, min_rays)[0] & ENOUGH else UNKNOWN)
        return out

    def forget(self, before_stamp=None, box=None):
        """box = (lo [3], hi [3]) in metres: voxel indices floor(bound / voxel_size), both faces' voxels included.  -> rows kept."""
        if box is not None:
            lo = [math.floor(float(v) / self.voxel_size) for v in box[0]]
            hi = [math.floor(float(v) / self.voxel_size) for v in box[1]]
        for c in list(self.rec):
            stale = before_stamp is not None and self.rec[c][2] < before_stamp
            outside = box is not None and not all(l <= v <= h for v, l, h in zip(c, lo, hi))
            if stale or outside:
                del self.rec[c]
        return len(self.rec)


def table_of(keys, rays, stamps):
    """The columns of a table (key order) as the restatement's dict: the KEY is decoded, none is formed."""
    out = {}
    for k, r, a, b in zip(np.asarray(keys).tolist(), np.asarray(rays).tolist(), np.asarray(stamps)[0].tolist(), np.asarray(stamps)[1].tolist()):
        out[((k >> 42) - BIAS, ((k >> 21) & 0x1fffff) - BIAS, (k & 0x1fffff) - BIAS)] = [r, a, b]
    return out
