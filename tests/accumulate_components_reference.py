"""Plain-Python restatement of the connected-components contract of the accumulated scene cloud (include/pcacc.h C11), the reference of
tests/test_accumulate_components.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]).  The voxels that take part
are held as a SET OF COORDINATES and a component is a breadth-first flood fill over the (2r+1)^3 offsets: no key is formed for a neighbour and no
row is searched, so a key whose field overflowed cannot alias another voxel here by accident.  Components are numbered by their smallest
(x, y, z) tuple; sums, boxes and stamps come from the records, as Python integers."""
from collections import deque

import numpy as np

from accumulate_prune_reference import BIAS, coord_of, keep, key_of

OK, BAD_MASK, GAVE_UP = 0, 1, 2
COUNTERS = ('rows', 'participating', 'outside', 'masked', 'components', 'largest', 'status')
REMOVE_COUNTERS = ('kept', 'small', 'components_removed', 'components_kept')


def kept_coords(ref_map, min_count=1, max_moving_fraction=None):
    """The coordinates extract() keeps, in its row order (ascending (x, y, z))."""
    return sorted(coord_of(k) for k, r in ref_map.rec.items() if keep(r[0], r[1], min_count, max_moving_fraction))


def flood(cells, radius):
    """cells: a set of coordinates -> a list of components (lists of coordinates), in ascending order of their smallest coordinate."""
    offsets = [(dx, dy, dz) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) for dz in range(-radius, radius + 1)]
    seen, out = set(), []
    for start in sorted(cells):
        if start in seen:
            continue
        seen.add(start)
        members, todo = [], deque([start])
        while todo:
            c = todo.popleft()
            members.append(c)
            for dx, dy, dz in offsets:
                n = (c[0] + dx, c[1] + dy, c[2] + dz)
                if all(-BIAS <= v < BIAS for v in n) and n in cells and n not in seen:
                    seen.add(n)
                    todo.append(n)
        out.append(members)
    return out


def components(ref_map, radius=1, min_count=1, max_moving_fraction=None, mask=None):
    """-> dict: label [kept] (extract's rows), per-component lists voxels, points, moving, sum_q, centroid (float32), lo, hi, t_first, t_last,
    first_row, and counters (COUNTERS order).  mask: a sequence over extract's rows, or None."""
    kept = kept_coords(ref_map, min_count, max_moving_fraction)
    rows = len(ref_map.rec)
    empty = dict(voxels=[], points=[], moving=[], sum_q=[], centroid=[], lo=[], hi=[], t_first=[], t_last=[], first_row=[])
    if mask is not None and len(mask) != len(kept):
        return dict(empty, label=[-1] * len(kept), counters=[rows, 0, rows - len(kept), len(kept), 0, 0, BAD_MASK])
    part = [c for j, c in enumerate(kept) if mask is None or mask[j]]
    row_of = {c: j for j, c in enumerate(kept)}
    label = [-1] * len(kept)
    out = dict(empty)
    for n, members in enumerate(flood(set(part), radius)):
        recs = [ref_map.rec[key_of(c)] for c in members]
        for c in members:
            label[row_of[c]] = n
        points = sum(r[0] for r in recs)
        sum_q = [sum(r[2 + a] for r in recs) for a in range(3)]
        out['voxels'].append(len(members))
        out['points'].append(points)
        out['moving'].append(sum(r[1] for r in recs))
        out['sum_q'].append(sum_q)
        out['centroid'].append([np.float32((np.float64(s) / np.float64(points)) * np.float64(2.0 ** -16)) for s in sum_q])
        out['lo'].append([min(c[a] for c in members) for a in range(3)])
        out['hi'].append([max(c[a] for c in members) for a in range(3)])
        out['t_first'].append(min(r[5] for r in recs))
        out['t_last'].append(max(r[6] for r in recs))
        out['first_row'].append(row_of[min(members)])
    out['label'] = label
    out['counters'] = [rows, len(part), rows - len(kept), len(kept) - len(part), len(out['voxels']), max(out['voxels'] or [0]), OK]
    return out


def small(voxels, points, min_voxels, min_points):
    return (min_voxels > 0 and voxels < min_voxels) or (min_points > 0 and points < min_points)


def remove_components(ref_map, pierced=None, min_voxels=0, min_points=0, dry_run=False, **args):
    """The counters [kept, small, components removed, components kept]; unless dry_run the voxels of the small components leave ref_map.rec and
    `pierced` ({coord: count} or None).  Voxels that do not take part stay."""
    res = components(ref_map, **args)
    kept = kept_coords(ref_map, args.get('min_count', 1), args.get('max_moving_fraction'))
    gone = [small(v, p, min_voxels, min_points) for v, p in zip(res['voxels'], res['points'])]
    leave = [c for c, lab in zip(kept, res['label']) if lab >= 0 and gone[lab]]
    counters = [len(ref_map.rec) - len(leave), len(leave), sum(gone), len(gone) - sum(gone)]
    if not dry_run and res['counters'][-1] == OK:
        for c in leave:
            del ref_map.rec[key_of(c)]
            if pierced is not None:
                pierced.pop(c, None)
    return counters
