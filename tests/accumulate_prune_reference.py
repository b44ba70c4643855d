"""Plain-Python restatement of the prune contract of the accumulated scene cloud (include/pcacc.h C8), the reference of tests/test_accumulate_prune.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]) and a {coord: pierced} dict.
Stage A is the contract's tests in their literal order on Python integers and floats (IEEE float64, never contracted); stage B looks the (2r+1)^3
offsets up in a SET OF COORDINATES.  No key is formed for a neighbour and no row is searched, so a key whose field overflowed cannot alias another
voxel here by accident."""
import math

BIAS = 1 << 20
KEPT, FILTER, STALE, BOX, PIERCED, ISOLATED = range(6)
NAMES = ('kept', 'filter', 'stale', 'box', 'pierced', 'isolated')


def coord_of(key):
    return ((key >> 42) - BIAS, ((key >> 21) & 0x1fffff) - BIAS, (key & 0x1fffff) - BIAS)


def key_of(c):
    return ((c[0] + BIAS) << 42) | ((c[1] + BIAS) << 21) | (c[2] + BIAS)


def box_indices(box, voxel_size):
    """(lo [3], hi [3]) in metres -> inclusive voxel indices: floor(bound / voxel_size) in float64, clamped into the grid."""
    index = lambda v: int(min(max(math.floor(float(v) / float(voxel_size)), -BIAS), BIAS - 1))
    return [index(v) for v in box[0]], [index(v) for v in box[1]]


def keep(count, moving, min_count, max_moving_fraction):
    """extract's predicate."""
    if count < min_count or count <= 0:
        return False
    if max_moving_fraction is not None and not float(moving) / float(count) <= float(max_moving_fraction):
        return False
    return True


def stage_a(r, coord, p, min_count=1, max_moving_fraction=None, before_stamp=None, box=None, min_pierced=0, ratio=None):
    """The reason of one record; box = (lo, hi) in voxel indices; p = the voxel's ray count, None without a sidecar."""
    if not keep(r[0], r[1], min_count, max_moving_fraction):
        return FILTER
    if before_stamp is not None and r[6] < before_stamp:
        return STALE
    if box is not None and any(coord[a] < box[0][a] or coord[a] > box[1][a] for a in range(3)):
        return BOX
    if min_pierced > 0 and p is not None and p >= min_pierced:
        if ratio is None or float(p) / float(r[0]) > float(ratio):
            return PIERCED
    return KEPT


def reasons(ref_map, pierced=None, min_neighbors=0, radius=1, **stage_a_args):
    """-> ({coord: reason}, {coord: k}) -- k for every stage-A survivor when min_neighbors > 0.  pierced: {coord: count} (a voxel it does not name has 0),
    or None = no sidecar."""
    why = {}
    for key, r in ref_map.rec.items():
        c = coord_of(key)
        why[c] = stage_a(r, c, None if pierced is None else pierced.get(c, 0), **stage_a_args)
    count = {}
    if min_neighbors > 0:
        alive = {c for c, w in why.items() if w == KEPT}
        for c in alive:
            k = 0
            for dx in range(-radius, radius + 1):
                for dy in range(-radius, radius + 1):
                    for dz in range(-radius, radius + 1):
                        n = (c[0] + dx, c[1] + dy, c[2] + dz)
                        if all(-BIAS <= v < BIAS for v in n) and n in alive:
                            k += 1
            count[c] = k
        for c, k in count.items():
            if k < min_neighbors:
                why[c] = ISOLATED
    return why, count


def prune(ref_map, pierced=None, dry_run=False, **args):
    """The counters [kept, filter, stale, box, pierced, isolated]; unless dry_run the removed voxels leave ref_map.rec and `pierced`."""
    why, _ = reasons(ref_map, pierced, **args)
    counters = [0] * 6
    for w in why.values():
        counters[w] += 1
    if not dry_run:
        for c, w in why.items():
            if w != KEPT:
                del ref_map.rec[key_of(c)]
                if pierced is not None:
                    pierced.pop(c, None)
    return counters
