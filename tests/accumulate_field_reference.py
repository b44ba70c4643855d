"""Brute-force restatement of the distance-field contract of the accumulated scene cloud (include/pcacc.h C19), the reference of
tests/test_accumulate_field.py.

It works on accumulate_reference.ReferenceMap.rec, whose keys are only unpacked into coordinates.  The sites of a box are a plain list of (coordinate,
row of extract); for every cell the squared distances to ALL sites are taken (a numpy broadcast over a block of cells), their minimum, the first site in
row order that attains it, and then the cut.  No pass along an axis, no packed value and no key is formed here, so neither a window cut wrongly at an
edge nor a tie decided by the order of a pass can enter by accident.  Everything is an integer."""
import numpy as np

import accumulate_columns_reference as cref
import accumulate_reference as ref

MAX_RADIUS, MAX_CELLS, MAX_ORIGIN = 128, 1 << 28, 1 << 31
VALID, INSIDE, NEAR = 1, 2, 4
BIAS = ref.BIAS


def cells_of(shape, planar):
    nx, ny, nz = shape
    return nx * ny * (1 if planar else nz)


def sites_of(rmap, origin, shape, planar=False, min_count=1, max_moving_fraction=None):
    """-> ([((x, y, z), row of extract)] of the kept voxels inside the box, ascending in row; the number of kept rows)."""
    rows = cref.kept_rows(rmap, min_count, max_moving_fraction)
    inside = [(c, j) for j, (c, _) in enumerate(rows) if all(origin[a] <= c[a] < origin[a] + shape[a] for a in range(3))]
    return inside, len(rows)


def field(rmap, origin, shape, max_radius, planar=False, min_count=1, max_moving_fraction=None):
    """-> dist2, nearest [nx, ny, nz or 1] i32, counters (a list of 4: kept rows, sites, cells with a result, cells without), sites (the number of
    voxels of the box, which is above the sites counter when a planar column holds two)."""
    R = int(max_radius)
    nx, ny, nz = (int(v) for v in shape)
    assert 1 <= R <= MAX_RADIUS and min(nx, ny, nz) >= 1 and cells_of(shape, planar) <= MAX_CELLS and all(abs(int(v)) <= MAX_ORIGIN for v in origin)
    nzo, axes = (1, 2) if planar else (nz, 3)
    dist2, nearest = np.full((nx, ny, nzo), -1, np.int32), np.full((nx, ny, nzo), -1, np.int32)
    if not rmap.rec:                                                                 # m = 0: all -1 and zero counters
        return dict(dist2=dist2, nearest=nearest, counters=[0, 0, 0, 0], voxels=0)
    inside, kept = sites_of(rmap, origin, shape, planar, min_count, max_moving_fraction)
    n_sites = len({c[:2] for c, _ in inside}) if planar else len(inside)
    if inside:
        s = np.array([c[:axes] for c, _ in inside], np.int64)                        # [S, axes], rows ascending
        row = np.array([j for _, j in inside], np.int64)
        grid = np.stack(np.meshgrid(*[np.arange(origin[a], origin[a] + (nx, ny, nzo)[a], dtype=np.int64) for a in range(axes)], indexing='ij'), -1)
        cells = grid.reshape(-1, axes)
        d2_out, row_out = np.empty(cells.shape[0], np.int64), np.empty(cells.shape[0], np.int64)
        step = max(1, (1 << 22) // s.shape[0])
        for a in range(0, cells.shape[0], step):
            e = cells[a:a + step, None, :] - s[None, :, :]
            d2 = (e * e).sum(-1)                                                     # [block, S]
            least = d2.min(1)
            first = (d2 == least[:, None]).argmax(1)                                 # the first site in row order at the minimum: the lowest row
            d2_out[a:a + step], row_out[a:a + step] = least, row[first]
        near = d2_out <= R * R
        dist2[...] = np.where(near, d2_out, -1).reshape(nx, ny, nzo)
        nearest[...] = np.where(near, row_out, -1).reshape(nx, ny, nzo)
    with_result = int((dist2 >= 0).sum())
    return dict(dist2=dist2, nearest=nearest, counters=[kept, n_sites, with_result, nx * ny * nzo - with_result], voxels=len(inside))


def voxels_of_points(points, pose, voxel_size):
    """[(x, y, z) or None] by C4's per-point arithmetic and validity rule."""
    valid, key, _ = ref.per_point(points, pose, voxel_size)
    return [((int(k) >> 42) - BIAS, ((int(k) >> 21) & 0x1fffff) - BIAS, (int(k) & 0x1fffff) - BIAS) if v else None for v, k in zip(valid, key)]


def voxels_of_coords(coords):
    return [tuple(int(v) for v in c) if all(-BIAS <= int(v) < BIAS for v in c) else None for c in np.asarray(coords).reshape(-1, 3)]


def lookup(voxels, f, origin, shape, planar=False):
    """voxels: [(x, y, z) or None = invalid]; f: a field() result on (origin, shape, planar) -> status u8, dist2, row i32 [n], counters (a list of 4)."""
    n = len(voxels)
    status, dist2, row = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for i, c in enumerate(voxels):
        if c is None:
            continue
        status[i] = VALID
        if not all(origin[a] <= c[a] < origin[a] + shape[a] for a in range(3)):
            continue
        status[i] |= INSIDE
        at = (c[0] - origin[0], c[1] - origin[1], 0 if planar else c[2] - origin[2])
        if f['dist2'][at] >= 0:
            status[i] |= NEAR
            dist2[i], row[i] = f['dist2'][at], f['nearest'][at]
    return dict(status=status, dist2=dist2, row=row,
                counters=[n, int((status & VALID != 0).sum()), int((status & INSIDE != 0).sum()), int((status & NEAR != 0).sum())])
