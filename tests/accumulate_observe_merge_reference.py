"""Plain-Python restatement of the merge and the regrid of observed space (include/pcacc.h C15), the reference of
tests/test_accumulate_observe_merge.py.

A table is accumulate_observe_reference.ReferenceSpace: a dict of voxel coordinates, (x, y, z) -> [rays, t_first, t_last], plus the five counters.  No key
is formed and nothing is sorted: a merge is a walk over two dicts, a regrid a dict update per row.  The pose arithmetic is numpy float64 in the header's
literal order of operations (no FMA: numpy has none)."""
import numpy as np

import accumulate_observe_reference as oref

BIAS = oref.BIAS
COORD_LIMIT = 32768.0


def merge(a, b):
    """A and B on one grid -> (the union as a NEW ReferenceSpace, {'rows', 'shared', 'new'}); neither is modified.  a may be b."""
    assert a.voxel_size == b.voxel_size
    out = oref.ReferenceSpace(a.voxel_size)
    shared = 0
    for c, r in a.rec.items():
        s = b.rec.get(c)
        if s is None:
            out.rec[c] = list(r)
        else:
            out.rec[c] = [r[0] + s[0], min(r[1], s[1]), max(r[2], s[2])]
            shared += 1
    for c, s in b.rec.items():
        if c not in a.rec:
            out.rec[c] = list(s)
    out.counters = [x + y for x, y in zip(a.counters, b.counters)]
    return out, dict(rows=len(out.rec), shared=shared, new=len(b.rec) - shared)


def landing(coords, pose, in_voxel_size, out_voxel_size):
    """Where the centres of the voxels `coords` [n,3] land: -> (valid [n] bool, indices [n,3] int64; rows that are not valid hold nothing).
    p_a = (float64(c_a) + 0.5) * in_voxel_size;  w_a = ((r_a0 * p_x + r_a1 * p_y) + r_a2 * p_z) + t_a;  valid iff every w_a is finite, |w_a| < 32768 and
    -2^20 <= floor(w_a / out_voxel_size) < 2^20."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    in_vs, out_vs = np.float64(in_voxel_size), np.float64(out_voxel_size)
    p = (c.astype(np.float64) + np.float64(0.5)) * in_vs
    valid = np.ones(c.shape[0], bool)
    idx = np.zeros(c.shape, np.int64)
    with np.errstate(all='ignore'):
        for a in range(3):
            w = ((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3]
            ok = np.isfinite(w) & (np.abs(w) < COORD_LIMIT)
            i = np.floor(w / out_vs)
            ok &= (i >= -float(BIAS)) & (i < float(BIAS))
            valid &= ok
            idx[:, a] = np.where(ok, i, 0).astype(np.int64)
    return valid, idx


def regrid(space, pose=None, voxel_size=None):
    """-> (a NEW ReferenceSpace at voxel_size (None = the same) under pose, the rows dropped).  Rows that land in one voxel fold to the maximum ray count,
    the minimum first stamp and the maximum last stamp; the counters are carried over."""
    out_vs = space.voxel_size if voxel_size is None else float(voxel_size)
    out = oref.ReferenceSpace(out_vs)
    out.counters = list(space.counters)
    coords = list(space.rec)
    if not coords:
        return out, 0
    valid, idx = landing(coords, pose, space.voxel_size, out_vs)
    dropped = 0
    for c, ok, d in zip(coords, valid.tolist(), idx.tolist()):
        if not ok:
            dropped += 1
            continue
        r, d = space.rec[c], tuple(d)
        have = out.rec.get(d)
        if have is None:
            out.rec[d] = list(r)
        else:
            out.rec[d] = [max(have[0], r[0]), min(have[1], r[1]), max(have[2], r[2])]
    return out, dropped


def columns(space):
    """The restatement's dict as the columns of a table in ascending key order: keys [m] i64, rays [m] i64, stamps [2,m] i32.  The one place a key is
    formed: to hand a table to the code under test."""
    rows = sorted(space.rec.items())                                             # ascending (x, y, z) = ascending keys
    keys = np.array([((c[0] + BIAS) << 42) | ((c[1] + BIAS) << 21) | (c[2] + BIAS) for c, _ in rows], np.int64)
    rays = np.array([r[0] for _, r in rows], np.int64)
    stamps = np.array([[r[1] for _, r in rows], [r[2] for _, r in rows]], np.int32).reshape(2, -1)
    return keys, rays, stamps
