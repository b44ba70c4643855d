"""numpy restatement of the per-voxel normals of the accumulated scene cloud (include/pcacc.h C5), the reference of tests/test_accumulate_normals.py,
on top of accumulate_reference.ReferenceMap.

A dict from voxel coordinates to row, the neighbour set as the contract defines it (Chebyshev radius r over the rows the extract filter keeps, offsets
that leave [-2^20, 2^20) skipped), the covariance of the float64 centroids in float64, np.linalg.eigh.  It does not share the kernel's operation order
or its decomposition: the claim against it carries a bound (eigenvalues, normals up to sign) or is an equality of integers (neighbours, flags)."""
import numpy as np

import accumulate_reference as ref

RANK_TOL = 64 * 2.0 ** -52
FEW, DEGENERATE, VIEWPOINT = 1, 2, 4


def kept_records(rmap, min_count=1, max_moving_fraction=None):
    """keys [V], acc [5,V], stamps [2,V] of the rows extract(min_count, max_moving_fraction) keeps, in key order."""
    keys, acc, stamps = rmap.records()
    keep = (acc[0] >= min_count) & (acc[0] > 0)
    if max_moving_fraction is not None:
        keep &= acc[1].astype(np.float64) / acc[0].astype(np.float64) <= np.float64(max_moving_fraction)
    return keys[keep], acc[:, keep], stamps[:, keep]


def neighbor_rows(coords, radius):
    """[(row, neighbour rows ascending)]: the participating voxels within Chebyshev distance `radius` of every voxel, itself included."""
    where = {tuple(c): j for j, c in enumerate(coords.tolist())}
    offsets = [(dx, dy, dz) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) for dz in range(-radius, radius + 1)]
    out = []
    for x, y, z in coords.tolist():
        rows = []
        for dx, dy, dz in offsets:
            n = (x + dx, y + dy, z + dz)
            if min(n) < -ref.BIAS or max(n) >= ref.BIAS:
                continue                                                         # out of the grid: no key exists for it
            j = where.get(n)
            if j is not None:
                rows.append(j)
        out.append(sorted(rows))                                                 # rows are in key order
    return out


def normals(rmap, radius=1, min_neighbors=5, min_count=1, max_moving_fraction=None, viewpoints=None, stamp_base=0):
    """-> dict: normals [V,3] f64 (zero where invalid), eigenvalues [V,3] f64 descending, neighbors [V] i32, flags [V] u8, gap [V] f64 =
    (lambda_mid - lambda_min) / lambda_max (0 where lambda_max is 0), centroids [V,3] f64."""
    keys, acc, stamps = kept_records(rmap, min_count, max_moving_fraction)
    v = keys.shape[0]
    coords = (np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - ref.BIAS).reshape(v, 3)
    cent = (acc[2:5].T.astype(np.float64) / acc[0].astype(np.float64)[:, None]) * np.float64(2.0 ** -16)
    nbr = neighbor_rows(coords, radius)
    k = np.array([len(r) for r in nbr], np.int32).reshape(v)
    cov = np.zeros((v, 3, 3))
    for i, rows in enumerate(nbr):
        d = cent[rows] - cent[i]
        mu = d.mean(0)
        cov[i] = (d[:, :, None] * d[:, None, :]).mean(0) - mu[:, None] * mu[None, :]
    w, vec = np.linalg.eigh(cov) if v else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    w = np.maximum(w, 0.0)                                                       # eigh may return -1e-20 for an exact zero
    eig = w[:, ::-1]
    n = vec[:, :, 0].copy()
    flags = np.zeros(v, np.uint8)
    flags[k < min_neighbors] |= FEW
    flags[eig[:, 1] <= RANK_TOL * eig[:, 0]] |= DEGENERATE
    valid = flags == 0
    n[~valid] = 0.0
    t = stamps[0].astype(np.int64) - int(stamp_base)
    if viewpoints is not None:
        vp = np.asarray(viewpoints, np.float64).reshape(-1, 3)
        use = valid & (t >= 0) & (t < vp.shape[0])
    else:
        vp, use = np.zeros((1, 3)), np.zeros(v, bool)
    toward = vp[np.where(use, t, 0)] - cent
    flip_vp = (n * toward).sum(1) < 0
    first = np.where(n[:, 2] != 0, n[:, 2], np.where(n[:, 1] != 0, n[:, 1], n[:, 0]))
    flip = np.where(use, flip_vp, first < 0)
    n[flip] = -n[flip]
    flags[use] |= VIEWPOINT
    with np.errstate(all='ignore'):
        gap = np.where(eig[:, 0] > 0, (eig[:, 1] - eig[:, 2]) / eig[:, 0], 0.0)
    return {'normals': n, 'eigenvalues': eig, 'neighbors': k, 'flags': flags, 'gap': gap, 'centroids': cent}
