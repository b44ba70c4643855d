"""Plain numpy restatement of the comparison of two accumulated scene clouds and of the selection of extract()'s rows by a mask (include/pcacc.h
C13), the reference of tests/test_accumulate_compare.py.  It works on ReferenceMap (tests/accumulate_reference.py) and on a {key: rays} dict for the
ray counts (None: no sidecar).  The float64 arithmetic is element-wise in the literal operation order of the contract; the 27 voxels around a row are
visited in ascending key order (dx, inside it dy, inside it dz) and a strict < keeps the first of equal distances.  The claim against it is equality:
integers directly, float64 as bits."""
import numpy as np

import accumulate_reference as ref

SAME, HELD, NEAR = 1, 2, 4
SIDE = ('rows', 'kept', 'same', 'held', 'near', 'only')
OK, BAD_MASK = 0, 1


def _keep(acc, min_count, max_moving_fraction):
    count, moving = acc[0], acc[1]
    keep = (count >= min_count) & (count > 0)
    if max_moving_fraction is not None:
        with np.errstate(all='ignore'):
            keep &= moving.astype(np.float64) / count.astype(np.float64) <= np.float64(max_moving_fraction)
    return keep


def _centroids(acc):
    """[3, M] float64: ((double)sum q / (double)count) * 2^-16."""
    return (acc[2:5].astype(np.float64) / acc[0].astype(np.float64)[None, :]) * np.float64(1.0 / ref.FIXED)


def _find(keys, wanted):
    """Position of every wanted key in the ascending `keys` and whether it is there."""
    if keys.shape[0] == 0:
        return np.zeros(wanted.shape, np.int64), np.zeros(wanted.shape, bool)
    q = np.searchsorted(keys, wanted)
    qc = np.minimum(q, keys.shape[0] - 1)
    return qc, (q < keys.shape[0]) & (keys[qc] == wanted)


def _side(own, other, other_rays, max_distance, min_count, max_moving_fraction):
    ok, oa, _ = own.records()
    tk, ta, _ = other.records()
    keep_o, keep_t = _keep(oa, min_count, max_moving_fraction), _keep(ta, min_count, max_moving_fraction)
    keys, w = ok[keep_o], _centroids(oa[:, keep_o])
    n = keys.shape[0]
    t_row = np.where(keep_t, np.cumsum(keep_t) - 1, -1)                          # the other's extract row of every row of the other
    q, held = _find(tk, keys)
    same = held & (keep_t[q] if tk.shape[0] else False)
    same_row = np.where(same, t_row[q] if tk.shape[0] else -1, -1)
    rays = np.zeros(tk.shape[0], np.int64) if other_rays is None else np.array([other_rays.get(int(k), 0) for k in tk.tolist()], np.int64)
    pierced = np.where(held, rays[q] if tk.shape[0] else 0, 0)
    kk, kc = tk[keep_t], _centroids(ta[:, keep_t])                               # the rows the other's extract returns
    idx = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff]) - ref.BIAS
    best_d2, best_row = np.zeros(n, np.float64), np.full(n, -1, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                c = idx + np.array([[dx], [dy], [dz]])
                inside = np.all((c >= -ref.BIAS) & (c < ref.BIAS), 0)            # an offset that leaves the grid forms no key
                c = np.where(inside, c, 0)
                p, hit = _find(kk, ((c[0] + ref.BIAS) << 42) | ((c[1] + ref.BIAS) << 21) | (c[2] + ref.BIAS))
                hit &= inside
                if not hit.any():
                    continue
                e = w - kc[:, p]
                d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                better = hit & ((best_row < 0) | (d2 < best_d2))
                best_d2, best_row = np.where(better, d2, best_d2), np.where(better, p, best_row)
    near = (best_row >= 0) & (best_d2 <= np.float64(max_distance) * np.float64(max_distance))
    status = (same * SAME + held * HELD + near * NEAR).astype(np.uint8)
    out = dict(status=status, same_row=same_row.astype(np.int32), row=np.where(near, best_row, -1).astype(np.int32),
               distance=np.where(near, np.sqrt(best_d2), np.inf).astype(np.float64), pierced=pierced.astype(np.int32))
    only = int(((status & (SAME | NEAR)) == 0).sum())
    return out, dict(rows=ok.shape[0], kept=n, same=int(same.sum()), held=int(held.sum()), near=int(near.sum()), only=only)


def compare(a, pa, b, pb, max_distance, min_count=1, max_moving_fraction=None):
    """Maps a and b (ReferenceMap, one voxel size; a may be b) with ray counts pa, pb -> {'self': columns, 'other': columns, 'counters': {side: dict}},
    one row per row of each map's extract(min_count, max_moving_fraction)."""
    assert a.voxel_size == b.voxel_size and 0.0 < max_distance <= a.voxel_size and min_count >= 1
    sa, ca = _side(a, b, pb, max_distance, min_count, max_moving_fraction)
    sb, cb = _side(b, a, pa, max_distance, min_count, max_moving_fraction)
    return {'self': sa, 'other': sb, 'counters': {'self': ca, 'other': cb}}


def select(a, pa, mask, invert=False, min_count=1, max_moving_fraction=None):
    """The rows of a.extract(min_count, max_moving_fraction) that `mask` names -> (the new ReferenceMap or None, its ray counts or None,
    [status, rows, kept, selected]).  A mask of the wrong length selects nothing: BAD_MASK and no map."""
    keys, acc, _ = a.records()
    kept = keys[_keep(acc, min_count, max_moving_fraction)]
    mask = np.asarray(mask)
    if mask.shape[0] != kept.shape[0]:
        return None, None, [BAD_MASK, keys.shape[0], kept.shape[0], 0]
    out = ref.ReferenceMap(a.voxel_size)
    po = None if pa is None else {}
    for k, flag in zip(kept.tolist(), mask.tolist()):
        if (flag != 0) != bool(invert):
            out.rec[k] = list(a.rec[k])
            if po is not None:
                po[k] = pa.get(k, 0)
    return out, po, [OK, keys.shape[0], kept.shape[0], len(out.rec)]
