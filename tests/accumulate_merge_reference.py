"""Plain numpy / Python restatement of the merge and the regrid of two accumulated scene clouds (include/pcacc.h C12), the reference of
tests/test_accumulate_merge.py.  It works on ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last] of Python integers) and
on a {key: rays} dict for the ray counts (None: no sidecar).  The float64 arithmetic of the regrid is element-wise in the literal operation order of the
contract (no `@`: BLAS may fuse).  The claim against it is equality."""
import numpy as np

import accumulate_reference as ref

PIERCED_MAX = (1 << 31) - 1
COUNT_MAX = 1 << 31


def merge(a, pa, b, pb):
    """Maps a and b (ReferenceMap, one voxel size) with ray counts pa, pb -> (the merged ReferenceMap, its ray counts or None, the result dict).
    Neither input is modified; a may be b."""
    assert a.voxel_size == b.voxel_size
    out = ref.ReferenceMap(a.voxel_size)
    out.dropped = a.dropped + b.dropped
    po = None if pa is None and pb is None else {}
    shared = new = saturated = 0
    for k, r in a.rec.items():
        out.rec[k] = list(r)
        if po is not None:
            po[k] = 0 if pa is None else pa.get(k, 0)
    for k, s in b.rec.items():
        r = a.rec.get(k)
        rays = 0 if pb is None else pb.get(k, 0)
        if r is None:
            new += 1
            out.rec[k] = list(s)
            if po is not None:
                po[k] = rays
        else:
            shared += 1
            out.rec[k] = [r[f] + s[f] for f in range(5)] + [min(r[5], s[5]), max(r[6], s[6])]
            if po is not None:
                total = po[k] + rays
                if total > PIERCED_MAX:
                    saturated += 1
                    total = PIERCED_MAX
                po[k] = total
    return out, po, dict(rows=len(out.rec), shared=shared, new=new, saturated=saturated)


def regrid(a, pa, pose, voxel_size):
    """Map a (ray counts pa or None) under `pose` ([4,4] or None) on a grid of voxel_size: every row as `count` points at its float64 centroid.
    -> (the new ReferenceMap, its ray counts or None, dict(rows_in, rows_out, dropped_rows, dropped_points, saturated))."""
    keys = sorted(a.rec)
    rows = np.array([a.rec[k] for k in keys], np.int64).reshape(-1, 7)
    count, moving = rows[:, 0], rows[:, 1]
    usable = (count > 0) & (count <= COUNT_MAX)
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    vs = np.float64(voxel_size)
    valid = usable.copy()
    idx, q = [], []
    with np.errstate(all='ignore'):
        c = [(rows[:, 2 + k].astype(np.float64) / count.astype(np.float64)) * np.float64(1.0 / ref.FIXED) for k in range(3)]
        for k in range(3):
            w = ((T[k, 0] * c[0] + T[k, 1] * c[1]) + T[k, 2] * c[2]) + T[k, 3]
            i = np.floor(w / vs)
            ok = np.isfinite(w) & (np.abs(w) < ref.LIMIT)
            ok &= (i >= -ref.BIAS) & (i < ref.BIAS)
            valid &= ok
            idx.append(np.where(ok, i, 0.0).astype(np.int64))
            q.append(np.where(ok, np.rint(w * ref.FIXED), 0.0).astype(np.int64))
    new_key = ((idx[0] + ref.BIAS) << 42) | ((idx[1] + ref.BIAS) << 21) | (idx[2] + ref.BIAS)
    out = ref.ReferenceMap(voxel_size)
    po = None if pa is None else {}
    dropped_rows = dropped_points = 0
    for j, k in enumerate(keys):
        n = int(count[j])
        if not valid[j]:
            dropped_rows += 1
            dropped_points += max(n, 0)
            continue
        nk = int(new_key[j])
        term = [n, int(moving[j])] + [n * int(q[ax][j]) for ax in range(3)]
        r = out.rec.get(nk)
        if r is None:
            out.rec[nk] = term + [int(rows[j, 5]), int(rows[j, 6])]
        else:
            out.rec[nk] = [r[f] + term[f] for f in range(5)] + [min(r[5], int(rows[j, 5])), max(r[6], int(rows[j, 6]))]
        if po is not None:
            po[nk] = po.get(nk, 0) + pa.get(k, 0)
    saturated = 0
    if po is not None:
        for nk, v in po.items():
            if v > PIERCED_MAX:
                saturated += 1
                po[nk] = PIERCED_MAX
    out.dropped = a.dropped + dropped_points
    return out, po, dict(rows_in=len(keys), rows_out=len(out.rec), dropped_rows=dropped_rows, dropped_points=dropped_points, saturated=saturated)


def aligned(pierced, keys):
    """The ray counts of a {key: rays} dict as the int32 column beside `keys`."""
    return np.array([pierced.get(int(k), 0) for k in np.asarray(keys).tolist()], np.int32)
