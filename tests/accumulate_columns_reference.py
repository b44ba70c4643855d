"""Plain-Python restatement of the column / ground / bird's-eye-view contract of the accumulated scene cloud (include/pcacc.h C17), the reference of
tests/test_accumulate_columns.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]), whose keys are only unpacked
into coordinates.  A column is a dict entry keyed by (x, y); the ground of a column is Python's min over the explicit tuples (z_low, (x', y')) of the
neighbours that exist, so the tie rule is the order of the tuples; a pixel is a dict lookup.  No key is formed, no sorted list is searched and no scan
runs, so neither a key whose field overflowed nor a run head that fell on a wave boundary can enter here by accident.  Arithmetic is Python floats
(IEEE float64, never contracted); np.float32 only for the final rounding of a pixel."""
import numpy as np

import accumulate_prune_reference as rref

BIAS = rref.BIAS
MAX_RADIUS, MAX_HEIGHT, MAX_PIXELS = 8, (1 << 21) - 1, 1 << 28
COLUMN_FIELDS = ('xy', 'first_row', 'voxels', 'points', 'moving', 'z_low', 'z_high', 't_first', 't_last', 'ground_z', 'ground_row', 'ground_column',
                 'band_voxels', 'band_top')
ROW_FIELDS = ('row_column', 'row_height', 'row_is_ground', 'row_height_m')
BEV_FIELDS = ('column', 'elevation', 'ground', 'band_top', 'voxels')
DTYPES = dict(xy=np.int32, first_row=np.int32, voxels=np.int32, points=np.int64, moving=np.int64, z_low=np.int32, z_high=np.int32, t_first=np.int32,
              t_last=np.int32, ground_z=np.int32, ground_row=np.int32, ground_column=np.int32, band_voxels=np.int32, band_top=np.int32,
              row_column=np.int32, row_height=np.int32, row_is_ground=np.uint8, row_height_m=np.float64,
              column=np.int32, elevation=np.float32, ground=np.float32)


def kept_rows(rmap, min_count=1, max_moving_fraction=None):
    """[((x, y, z), record)] of the voxels the filter keeps, in ascending (x, y, z): position = extract's row."""
    out = [(rref.coord_of(key), r) for key, r in rmap.rec.items() if rref.keep(r[0], r[1], min_count, max_moving_fraction)]
    out.sort(key=lambda t: t[0])
    return out


def _z64(r):
    return (float(r[4]) / float(r[0])) * (1.0 / 65536.0)


def columns(rmap, ground_radius=2, thickness=1, band=(2, 20), min_count=1, max_moving_fraction=None):
    """-> dict of numpy tables (COLUMN_FIELDS with C rows, ROW_FIELDS with V rows), 'counters' (a list of 5), 'kept' and 'n_columns'."""
    R, (lo, hi) = int(ground_radius), band
    assert 0 <= R <= MAX_RADIUS and 0 <= thickness <= MAX_HEIGHT and 0 <= lo <= hi <= MAX_HEIGHT
    rows = kept_rows(rmap, min_count, max_moving_fraction)
    cols = {}                                                                       # (x, y) -> [(z, row of extract, record)]
    for j, ((x, y, z), r) in enumerate(rows):
        cols.setdefault((x, y), []).append((z, j, r))
    order = sorted(cols)
    number = {xy: c for c, xy in enumerate(order)}
    z_low = {xy: min(v[0] for v in vox) for xy, vox in cols.items()}
    first = {xy: min(v[1] for v in vox) for xy, vox in cols.items()}
    V, C = len(rows), len(order)
    out = {f: np.zeros((C, 2) if f == 'xy' else (C,), DTYPES[f]) for f in COLUMN_FIELDS}
    out.update({f: np.zeros((V,), DTYPES[f]) for f in ROW_FIELDS})
    borrowed = 0
    for c, (x, y) in enumerate(order):
        vox = cols[(x, y)]
        near = [(x + dx, y + dy) for dx in range(-R, R + 1) for dy in range(-R, R + 1)]
        near = [n for n in near if -BIAS <= n[0] < BIAS and -BIAS <= n[1] < BIAS and n in cols]
        gz, supplier = min((z_low[n], n) for n in near)                             # (x, y) order IS column-key order
        borrowed += supplier != (x, y)
        heights = [z - gz for z, _, _ in vox]
        inside = [h for h in heights if lo <= h <= hi]
        out['xy'][c] = (x, y)
        out['first_row'][c], out['voxels'][c] = first[(x, y)], len(vox)
        out['points'][c], out['moving'][c] = sum(v[2][0] for v in vox), sum(v[2][1] for v in vox)
        out['z_low'][c], out['z_high'][c] = z_low[(x, y)], max(v[0] for v in vox)
        out['t_first'][c], out['t_last'][c] = min(v[2][5] for v in vox), max(v[2][6] for v in vox)
        out['ground_z'][c], out['ground_row'][c], out['ground_column'][c] = gz, first[supplier], number[supplier]
        out['band_voxels'][c], out['band_top'][c] = len(inside), max(inside) if inside else -1
        for z, j, r in vox:
            out['row_column'][j], out['row_height'][j], out['row_is_ground'][j] = c, z - gz, 1 if z - gz <= thickness else 0
            out['row_height_m'][j] = _z64(r) - _z64(rows[first[supplier]][1])
    out['counters'] = [V, C, int(out['row_is_ground'].sum()), int(out['band_voxels'].sum()), borrowed]
    out['kept'], out['n_columns'] = V, C
    out['_rows'], out['_number'] = rows, number
    return out


def bev(cols, origin, shape):
    """The images of the window at origin = (x0, y0) of shape = (H, W) from a columns() result -> dict of BEV_FIELDS arrays [H, W]."""
    (x0, y0), (H, W) = origin, shape
    assert H >= 1 and W >= 1 and H * W <= MAX_PIXELS
    out = dict(column=np.full((H, W), -1, np.int32), elevation=np.full((H, W), np.nan, np.float32), ground=np.full((H, W), np.nan, np.float32),
               band_top=np.full((H, W), -1, np.int32), voxels=np.zeros((H, W), np.int32))
    rows, number = cols['_rows'], cols['_number']
    for r in range(H):
        for c in range(W):
            k = number.get((x0 + c, y0 + r))
            if k is None:
                continue
            out['column'][r, c] = k
            out['elevation'][r, c] = np.float32(_z64(rows[int(cols['first_row'][k]) + int(cols['voxels'][k]) - 1][1]))
            out['ground'][r, c] = np.float32(_z64(rows[int(cols['ground_row'][k])][1]))
            out['band_top'][r, c], out['voxels'][r, c] = cols['band_top'][k], cols['voxels'][k]
    return out


def bounding_box(cols):
    """origin (x0, y0) and shape (H, W) of the columns; (0, 0), (1, 1) without one."""
    if cols['n_columns'] == 0:
        return (0, 0), (1, 1)
    lo, hi = cols['xy'].min(0), cols['xy'].max(0)
    return (int(lo[0]), int(lo[1])), (int(hi[1] - lo[1]) + 1, int(hi[0] - lo[0]) + 1)
