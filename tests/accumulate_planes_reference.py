"""Plain-Python restatement of the planar-segment contract of the accumulated scene cloud (include/pcacc.h C18), the reference of
tests/test_accumulate_planes.py.

It works on accumulate_reference.ReferenceMap.rec (key -> [count, moving, sum q_x, sum q_y, sum q_z, t_first, t_last]) and on GIVEN normal,
eigenvalue and flag arrays over extract's rows, so a label never depends on an eigen-solver.  The voxels that take part are a dict of coordinates;
a segment is a breadth-first fill over the (2r+1)^3 offsets in which a step is taken only where the edge rule holds, the rule in numpy float64
scalars in the contract's order of operations.  No key is formed for a neighbour and there is no union-find.  Segments are numbered by their
smallest (x, y, z); the moments D, s, S1, S2 are Python integers; the plane comes from np.linalg.eigh on the covariance formed EXACTLY (fractions)
from those integers: the claim against it carries a bound."""
from collections import deque
from fractions import Fraction

import numpy as np

from accumulate_components_reference import kept_coords
from accumulate_prune_reference import BIAS, key_of

OK, BAD_ROWS, GAVE_UP = 0, 1, 2
COUNTERS = ('rows', 'participating', 'outside', 'masked', 'invalid', 'not_flat', 'segments', 'largest', 'status')
FEW, DEGENERATE = 1, 2
PLANE_DEGENERATE = 1
RANK_TOL = 64 * 2.0 ** -52
INT_TABLES = (('voxels', np.int32, ()), ('points', np.int64, ()), ('lo', np.int32, (3,)), ('hi', np.int32, (3,)), ('first_row', np.int32, ()),
              ('t_first', np.int32, ()), ('t_last', np.int32, ()), ('anchor', np.int32, (3,)), ('spread', np.int64, ()), ('shift', np.int32, ()),
              ('s1', np.int64, (3,)), ('s2', np.int64, (6,)))
FIT_TABLES = (('normal', np.float64, (3,)), ('eigenvalues', np.float64, (3,)), ('centroid', np.float64, (3,)), ('offset', np.float64, ()),
              ('mse', np.float64, ()), ('flags', np.uint8, ()))
F64 = np.float64


def flat(e, max_variation):
    e0, e1, e2 = F64(e[0]), F64(e[1]), F64(e[2])
    with np.errstate(all='ignore'):
        return bool(e2 <= F64(max_variation) * ((e0 + e1) + e2))


def centroid(rec):
    return [(F64(rec[2 + a]) / F64(rec[0])) * F64(2.0 ** -16) for a in range(3)]


def joined(ni, ci, nj, cj, cos_angle, max_offset):
    """The edge rule between two rows: normals as float64 scalars (from the given float32), centroids float64."""
    dot = (ni[0] * nj[0] + ni[1] * nj[1]) + ni[2] * nj[2]
    if not abs(dot) >= F64(cos_angle):
        return False
    d = [cj[a] - ci[a] for a in range(3)]
    if not abs((ni[0] * d[0] + ni[1] * d[1]) + ni[2] * d[2]) <= F64(max_offset):
        return False
    return bool(abs((nj[0] * d[0] + nj[1] * d[1]) + nj[2] * d[2]) <= F64(max_offset))


def shift_of(spread, voxels):
    s = 0
    while not ((spread >> s) + 1 <= 2 ** 31 and ((spread >> s) + 1) ** 2 <= 2 ** 62 // voxels):
        s += 1
    return s


def fit(anchor, s, voxels, s1, s2):
    """np.linalg.eigh on the exact covariance of the integer moments -> normal (first non-zero of (n_z, n_y, n_x) positive), eigenvalues descending
    (m^2), centroid (m), offset, mse, flags, gap = (l_mid - l_min) / l_max."""
    n = voxels
    idx = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    cov = np.array([[float(Fraction(n * s2[idx[a][b]] - s1[a] * s1[b], n * n)) for b in range(3)] for a in range(3)], F64)
    w, vec = np.linalg.eigh(cov)
    w = np.maximum(w, 0.0)[::-1]
    scale2 = F64(2.0) ** (2 * (s - 16))
    eig = w * scale2
    cen = np.array([float(Fraction(anchor[a] * n + s1[a] * 2 ** s, n * 65536)) for a in range(3)], F64)
    gap = float((w[1] - w[2]) / w[0]) if w[0] > 0 else 0.0
    if w[1] <= RANK_TOL * w[0]:
        return dict(normal=np.zeros(3), eigenvalues=eig, centroid=cen, offset=0.0, mse=0.0, flags=PLANE_DEGENERATE, gap=gap)
    nrm = vec[:, 0].copy()
    first = nrm[2] if nrm[2] != 0 else (nrm[1] if nrm[1] != 0 else nrm[0])
    if first < 0:
        nrm = -nrm
    return dict(normal=nrm, eigenvalues=eig, centroid=cen, offset=float(nrm @ cen), mse=float(eig[2]), flags=0, gap=gap)


def planes(ref_map, normals, eigenvalues, flags, radius=1, cos_angle=1.0, max_offset=0.0, max_variation=1.0, min_count=1, max_moving_fraction=None,
           mask=None):
    """-> dict: label [kept], klass [kept] (0 takes part, -2 masked, -3 invalid normal, -4 not flat), the INT_TABLES as lists, fits (a list of
    fit() dicts), members (lists of coordinates) and counters (COUNTERS order).  normals, eigenvalues [n,3], flags [n]: given arrays over extract's
    rows; mask: a sequence over them, or None."""
    kept = kept_coords(ref_map, min_count, max_moving_fraction)
    rows = len(ref_map.rec)
    out = {name: [] for name, _, _ in INT_TABLES}
    out.update(fits=[], members=[])
    if len(normals) != len(kept) or len(eigenvalues) != len(kept) or len(flags) != len(kept) or (mask is not None and len(mask) != len(kept)):
        return dict(out, label=[-1] * len(kept), klass=[-2] * len(kept), counters=[rows, 0, rows - len(kept), len(kept), 0, 0, 0, 0, BAD_ROWS])
    klass = []
    for j in range(len(kept)):
        if mask is not None and not mask[j]:
            klass.append(-2)
        elif int(flags[j]) & (FEW | DEGENERATE):
            klass.append(-3)
        elif not flat(eigenvalues[j], max_variation):
            klass.append(-4)
        else:
            klass.append(0)
    row_of = {c: j for j, c in enumerate(kept)}
    part = {c: j for j, c in enumerate(kept) if klass[j] == 0}
    nrm = {c: [F64(v) for v in normals[j]] for c, j in part.items()}
    cen = {c: centroid(ref_map.rec[key_of(c)]) for c in part}
    offsets = [(dx, dy, dz) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) for dz in range(-radius, radius + 1)]
    seen, label = set(), [-1] * len(kept)
    for start in sorted(part):
        if start in seen:
            continue
        seen.add(start)
        members, todo = [], deque([start])
        while todo:
            c = todo.popleft()
            members.append(c)
            for dx, dy, dz in offsets:
                n = (c[0] + dx, c[1] + dy, c[2] + dz)
                if all(-BIAS <= v < BIAS for v in n) and n in part and n not in seen and joined(nrm[c], cen[c], nrm[n], cen[n], cos_angle, max_offset):
                    seen.add(n)
                    todo.append(n)
        k = len(out['voxels'])
        recs = [ref_map.rec[key_of(c)] for c in members]
        for c in members:
            label[row_of[c]] = k
        u = [[r[2 + a] // r[0] for a in range(3)] for r in recs]                  # Python's // is the floor
        anchor = u[members.index(min(members))]
        spread = max(abs(v[a] - anchor[a]) for v in u for a in range(3))
        s = shift_of(spread, len(members))
        e = [[(v[a] - anchor[a]) >> s for a in range(3)] for v in u]
        s1 = [sum(v[a] for v in e) for a in range(3)]
        s2 = [sum(v[a] * v[b] for v in e) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        assert len(members) * ((spread >> s) + 1) ** 2 <= 2 ** 62 and all(abs(v) < 2 ** 63 for v in s1 + s2)
        for name, value in (('voxels', len(members)), ('points', sum(r[0] for r in recs)), ('lo', [min(c[a] for c in members) for a in range(3)]),
                            ('hi', [max(c[a] for c in members) for a in range(3)]), ('first_row', row_of[min(members)]),
                            ('t_first', min(r[5] for r in recs)), ('t_last', max(r[6] for r in recs)), ('anchor', anchor), ('spread', spread),
                            ('shift', s), ('s1', s1), ('s2', s2)):
            out[name].append(value)
        out['fits'].append(fit(anchor, s, len(members), s1, s2))
        out['members'].append(members)
    out.update(label=label, klass=klass)
    count = lambda v: sum(1 for k in klass if k == v)
    out['counters'] = [rows, count(0), rows - len(kept), count(-2), count(-3), count(-4), len(out['voxels']), max(out['voxels'] or [0]), OK]
    return out

