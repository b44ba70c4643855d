"""Adversarial scenes for the test-mode clustering (csrc/cluster.hip), used by tests/test_cluster_edges.py.

A Scene is what the clustering SEES: float32 (x, y, z) per point, the selection, the sample index, a tag per point that says
what the builder meant the point to be, and a `check` that asserts -- on the reference's result -- that the scene still contains
the situation it was built for.  variant() turns a scene into the arrays of one call: one of the 8 symmetries of the square,
the split of the seen position into point + offset (use_offset) or a point and an offset that must be ignored, and a random
order inside every sample.  Every scene comes from a seed or a formula; nothing is read from disk."""
import functools
import itertools

import numpy as np

import oracle

MIN_SAMPLES = 5
SYMS = list(itertools.product((False, True), repeat=3))          # (flip x, flip y, transpose)
UNSEL = -1                                                       # tag of a point that is not selected


class Scene:
    def __init__(self, name, eps, xy, z, batch, tag, check, sel=None, n_batches=None):
        self.name, self.eps, self.check = name, float(eps), check
        self.xy = np.ascontiguousarray(xy, np.float32)
        self.z = np.ascontiguousarray(z, np.float32)
        self.batch = np.asarray(batch, np.int64)
        self.tag = np.asarray(tag, np.int64)
        self.sel = (self.tag != UNSEL) if sel is None else np.asarray(sel, bool)
        self.n_batches = n_batches
        assert self.xy.shape == (len(self.z), 2) and len(self.batch) == len(self.z) == len(self.tag) == len(self.sel)
        assert np.all(np.diff(self.batch) >= 0)                  # grouped by ascending sample index, as the collate gives them


class Variant:
    """The arrays of one call and the tags that go with them."""

    def __init__(self, scene, sym, use_offset, points, offset, mos, ti, tag):
        self.scene, self.eps, self.sym, self.use_offset = scene, scene.eps, sym, use_offset
        self.points, self.offset, self.mos, self.ti, self.tag = points, offset, mos, ti, tag
        for a in (points, offset, mos, ti, tag):
            a.setflags(write=False)

    @property
    def voxel(self):
        return 0.05 if self.use_offset else 0.15

    def seen(self):
        p = self.points.copy()
        if self.use_offset:
            p[:, :2] += self.offset
        return p


def variant(scene, sym, use_offset, seed):
    rng = np.random.RandomState(seed)
    flip_x, flip_y, transpose = sym
    t = scene.xy.copy()
    if flip_x:
        t[:, 0] = -t[:, 0]
    if flip_y:
        t[:, 1] = -t[:, 1]
    if transpose:
        t = t[:, ::-1].copy()
    n = len(t)
    if use_offset:
        # multiples of 1/64: point + offset gives the seen position back exactly wherever it can; where float32 cannot, no offset
        off = (rng.randint(-16, 17, (n, 2)) / 64.0).astype(np.float32)
        p = (t - off).astype(np.float32)
        bad = (p + off).astype(np.float32) != t
        off[bad] = 0
        p[bad] = t[bad]
        assert np.array_equal((p + off).astype(np.float32), t)
    else:
        off = (rng.randn(n, 2) * 0.5).astype(np.float32)           # must be ignored
        p = t
    order = np.concatenate([np.flatnonzero(scene.batch == b)[rng.permutation(int((scene.batch == b).sum()))]
                            for b in np.unique(scene.batch)]) if n else np.zeros(0, np.int64)
    points = np.concatenate([p, scene.z[:, None]], 1).astype(np.float32)[order]
    ti = np.stack([scene.batch, np.zeros(n, np.int64)], 1)[order]
    return Variant(scene, sym, use_offset, points, off[order].copy(), scene.sel.astype(np.int64)[order], ti, scene.tag[order].copy())


def reference(v, min_p_cluster, estimator=None, mos=None):
    """oracle.cluster_forward on the samples inside [0, n_batches); points of other sample indices are ignored -> 0."""
    mos = v.mos if mos is None else mos
    b = v.ti[:, 0]
    nb = v.scene.n_batches if v.scene.n_batches is not None else (int(b.max()) + 1 if len(b) else 1)
    ok = (b >= 0) & (b < nb)
    out = np.zeros(len(b), np.int64)
    if ok.any():
        out[ok] = oracle.cluster_forward(v.points[ok], mos[ok], v.offset[ok], v.ti[ok], v.eps, MIN_SAMPLES, min_p_cluster, v.use_offset,
                                         estimator=estimator)
    return out


# ---------------------------------------------------------------------------------------------------------------- analysis
def kept_voxels(src, voxel, rnd=np.round):
    """models/cluster.py:9-13 with a choice of rounding: indices of the kept points and the inverse map."""
    return oracle.sparse_quantize(rnd(np.asarray(src) / voxel))


def round_half_up(a):
    return np.floor(a + np.float32(0.5))


class Analysis:
    """Core / border / noise of one sample's selected points, by the reference's own steps: the kept points of the voxel down-sampling
    and the float64 test dx*dx + dy*dy <= eps*eps on them."""

    def __init__(self, v, sample):
        m = (v.ti[:, 0] == sample) & (v.mos == 1)
        self.rows = np.flatnonzero(m)
        src = v.seen()[m]
        self.sub, self.inv = kept_voxels(src, v.voxel)
        k = src[self.sub][:, :2].astype(np.float64)
        self.kxy = k
        dx = k[:, None, 0] - k[None, :, 0]
        d = dx * dx
        dy = k[:, None, 1] - k[None, :, 1]
        d = d + dy * dy
        self.near = d <= v.eps * v.eps
        self.core = self.near.sum(1) >= MIN_SAMPLES
        self.border = ~self.core & (self.near & self.core[None, :]).any(1)
        self.noise = ~self.core & ~self.border
        self.tag = v.tag[self.rows][self.sub]

    def labels(self, lab):
        """The label of every kept point out of a per-point label vector."""
        return lab[self.rows][self.sub]


def _labels_are_ranks(v, lab):
    """Labels restart at 1 in every sample and have no holes."""
    for b in np.unique(v.ti[:, 0]):
        u = np.unique(lab[v.ti[:, 0] == b])
        u = u[u > 0]
        assert np.array_equal(u, np.arange(1, len(u) + 1)), (b, u)


def _sprinkle_unselected(rng, xy, z, batch, tag, frac=0.1):
    """Points that are not selected, inside the bounding box of every sample: the clustering must not see them."""
    out = [(xy, z, batch, tag)]
    for b in np.unique(batch):
        m = batch == b
        k = max(3, int(frac * m.sum()))
        lo, hi = xy[m].min(0) - 1, xy[m].max(0) + 1
        out.append((rng.uniform(lo, hi, (k, 2)), rng.uniform(-1.5, 0.5, k), np.full(k, b), np.full(k, UNSEL)))
    xy, z, batch, tag = (np.concatenate([o[i] for o in out]) for i in range(4))
    order = np.argsort(batch, kind='stable')
    return xy[order], z[order], batch[order], tag[order]


# ------------------------------------------------------------------------------------------------- 1, 2: lattices
INTERIOR, EDGE, CORNER = 0, 1, 2
DYADIC = ((0.0, 0.0), (0.0625, 13.125), (13.125, -74.875), (-74.875, 0.0625))


def lattice(nx, ny, sx, sy, tx, ty):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    xy = np.stack([tx + sx * i.ravel(), ty + sy * j.ravel()], 1)
    on_x, on_y = (i == 0) | (i == nx - 1), (j == 0) | (j == ny - 1)
    tag = np.where(on_x & on_y, CORNER, np.where(on_x | on_y, EDGE, INTERIOR)).ravel()
    return xy, tag


def _lattice_scene(name, eps, sx, sy, translations, check, nx=24, ny=17, seed=0):
    rng = np.random.RandomState(seed)
    parts = [lattice(*(tuple(t[2:]) or (nx, ny)), sx, sy, t[0], t[1]) for t in translations]      # (tx, ty) or (tx, ty, nx, ny)
    xy = np.concatenate([p[0] for p in parts])
    tag = np.concatenate([p[1] for p in parts])
    batch = np.repeat(np.arange(len(parts)), [len(p[1]) for p in parts])
    z = rng.uniform(-1.5, 0.5, len(xy))
    return Scene(name, eps, *_sprinkle_unselected(rng, xy, z, batch, tag), check=check)


def _check_exact(v, lab, nx=24, ny=17):
    """Interior points have exactly min_samples neighbours (4 at distance exactly eps, and themselves): all core; edge points are
    border points; the four corners are noise."""
    _labels_are_ranks(v, lab)
    for b in np.unique(v.ti[:, 0]):
        a = Analysis(v, b)
        assert len(a.sub) == nx * ny                                              # no two lattice points share a voxel
        assert a.near.sum(1)[a.tag == INTERIOR].min() == a.near.sum(1)[a.tag == INTERIOR].max() == MIN_SAMPLES
        assert a.core[a.tag == INTERIOR].all() and not a.core[a.tag != INTERIOR].any()
        assert a.noise.sum() == 4 and a.noise[a.tag == CORNER].all()
        assert a.border.sum() == 2 * (nx + ny) - 4 - 4
        kl = a.labels(lab)
        assert (kl[a.noise] == 0).all() and (kl[~a.noise] == 1).all()


def _check_345(v, lab, nx=24, ny=17):
    """Spacing (0.375, 0.5), eps 0.625: the diagonal neighbour lies at squared distance exactly eps^2.  With it an edge point has 6
    neighbours (core) and a corner 4 (a border point); without it the edge points are border points and the corners noise."""
    _labels_are_ranks(v, lab)
    for b in np.unique(v.ti[:, 0]):
        a = Analysis(v, b)
        assert len(a.sub) == nx * ny
        cnt = a.near.sum(1)
        assert (cnt[a.tag == INTERIOR] == 9).all() and (cnt[a.tag == EDGE] == 6).all() and (cnt[a.tag == CORNER] == 4).all()
        d2 = ((a.kxy[:, None] - a.kxy[None]) ** 2).sum(2)
        assert (d2 == v.eps * v.eps).sum() >= 4 * (nx - 1) * (ny - 1)            # the diagonals are exact ties
        assert a.border.sum() == 4 and a.border[a.tag == CORNER].all() and a.noise.sum() == 0
        assert (a.labels(lab) == 1).all()


def _check_straddle(v, lab):
    """Neighbouring lattice points fall one ulp either side of eps: the lattice breaks into fragments, in every sample."""
    _labels_are_ranks(v, lab)
    for b in np.unique(v.ti[:, 0]):
        m = (v.ti[:, 0] == b) & (v.mos == 1)
        assert lab[m].max() > 1 and (lab[m] == 0).any(), (b, lab[m].max())
        a = Analysis(v, b)
        d2 = ((a.kxy[:, None] - a.kxy[None]) ** 2).sum(2)
        r2 = v.eps * v.eps
        just = np.abs(d2 - r2) < 1e-5 * r2                                     # lattice neighbours
        assert (just & (d2 <= r2)).any() and (just & (d2 > r2)).any()


# ------------------------------------------------------------------------------------------------- 3: shared border point
LAT_A, LAT_B, SHARED = 1, 2, 3


def _shared_border_scene():
    """Two 0.25-lattices A (columns 0..5, rows 0..7) and B (columns 7..12, rows -3..9) with eps = 0.25, and points P in the empty
    column 6 on rows 2, 4 and 6.  P has 3 neighbours (not core), makes its neighbour in A and its neighbour in B core, and is in
    range of both.  B reaches further down than A, so that after a transpose B holds the lowest voxel rank (cluster 1) although a
    scan in ascending cell order meets A first."""
    s = 0.25
    rng = np.random.RandomState(3)
    pts, tag = [], []
    for tx, ty in ((-3.0, 1.5), (41.125, -70.0)):
        for i in range(6):
            for j in range(8):
                pts.append((tx + s * i, ty + s * j)), tag.append(LAT_A)
        for i in range(7, 13):
            for j in range(-3, 10):
                pts.append((tx + s * i, ty + s * j)), tag.append(LAT_B)
        for j in (2, 4, 6):
            pts.append((tx + s * 6, ty + s * j)), tag.append(SHARED)
    xy, tag = np.array(pts), np.array(tag)
    batch = np.repeat([0, 1], len(xy) // 2)
    return Scene('shared_border', s, *_sprinkle_unselected(rng, xy, rng.uniform(-1.5, 0.5, len(xy)), batch, tag), check=_check_shared)


def _check_shared(v, lab):
    _labels_are_ranks(v, lab)
    for b in np.unique(v.ti[:, 0]):
        a = Analysis(v, b)
        kl = a.labels(lab)
        la, lb = np.unique(kl[(a.tag == LAT_A) & a.core]), np.unique(kl[(a.tag == LAT_B) & a.core])
        assert len(la) == 1 and len(lb) == 1 and la[0] != lb[0] and min(la[0], lb[0]) == 1          # A and B stay apart
        p = a.tag == SHARED
        assert p.sum() >= 3 and not a.core[p].any() and (a.near[p].sum(1) == 3).all()
        for row in np.flatnonzero(p):                                                               # in range of a core point of each
            assert set(kl[a.near[row] & a.core]) == {la[0], lb[0]}
        assert (kl[p] == min(la[0], lb[0])).all()


# ------------------------------------------------------------------------------------------------- 4: long thin components
def _spiral(n, ds, pitch, phase, r0):
    """n points along r = r0 + pitch * (theta - phase) / 2 pi, ds apart along the curve."""
    a = pitch / (2 * np.pi)
    th, out = 0.0, np.empty((n, 2))
    for k in range(n):
        r = r0 + a * th
        out[k] = r * np.cos(th + phase), r * np.sin(th + phase)
        th += ds / np.hypot(r, a)
    return out


def _spiral_scene(arms):
    """Points 0.13 apart along a spiral whose turns are 1.0 (one arm) or 0.5 (two interleaved arms) apart, eps = 0.4: a component a
    few thousand grid cells long and one cell wide."""
    rng = np.random.RandomState(4 + arms)
    n = 6000 // arms
    xy = np.concatenate([_spiral(n, 0.13, 1.0, np.pi * k, 1.0) for k in range(arms)]) + (31.7, -48.3)
    tag = np.repeat(np.arange(1, arms + 1), n)
    z = rng.uniform(-1.5, 0.5, len(xy))
    return Scene('spiral%d' % arms, 0.4, *_sprinkle_unselected(rng, xy, z, np.zeros(len(xy), np.int64), tag, 0.02),
                 check=functools.partial(_check_spiral, arms=arms))


def _check_spiral(v, lab, arms):
    _labels_are_ranks(v, lab)
    sel = v.mos == 1
    seen = v.seen()[:, :2].astype(np.float64)
    cell = 0.7 * v.eps
    big = []
    for arm in range(1, arms + 1):
        m = sel & (v.tag == arm)
        top = np.bincount(lab[m]).argmax()
        assert top > 0 and (lab[m] == top).mean() >= 0.9                       # one cluster holds the arm
        cells = np.unique(np.floor(seen[m & (lab == top)] / cell), axis=0)
        assert len(cells) > 1000 // arms * 1.5, len(cells)                     # ... and is thousands of cells long
        big.append(top)
    assert len(set(big)) == arms                                                # interleaved arms stay apart
    if arms == 1:
        assert (lab[sel] == big[0]).mean() >= 0.9 and len(np.unique(np.floor(seen[sel & (lab == big[0])] / cell), axis=0)) > 1000


# ------------------------------------------------------------------------------------------------- 5: poles and dense cells
POLE, SATELLITE, CORNER_GROUP, CORNER_FAR = 1, 2, 3, 4


def _poles_scene():
    """Poles of 30 points within 1 cm in (x, y), 0.2 apart in z: many voxels in one grid cell.  Each has 1-3 satellites just inside eps
    of 2-3 of its members and just outside eps of the rest, which makes them border points of a dense cell.  Some poles sit across
    a cell boundary.  The corner groups hold 5 stacked points and a single point at 1.002 eps along a diagonal, both inside one
    square of f * eps for f = 0.72 .. 0.80: noise as long as nobody takes a square that wide for a cell."""
    eps = 0.4
    cell = 0.7 * eps
    rng = np.random.RandomState(5)
    xy, z, tag = [], [], []
    for k in range(40):
        c = rng.uniform(-60, 60, 2)
        if k % 2:
            c = np.round(c / cell) * cell + (-0.004, rng.uniform(0.05, 0.2))       # members straddle a cell boundary in x
        rot = rng.uniform(0, 2 * np.pi) if k % 2 == 0 else 0.0
        n_sat = 1 + k % 3
        members = np.tile(c, (30, 1))
        used = 0
        for s in range(n_sat):
            u = np.array([np.cos(rot + 2 * np.pi * s / 3), np.sin(rot + 2 * np.pi * s / 3)])
            m = 2 + (k + s) % 2                                                  # 2 or 3 members shifted 8 mm towards the satellite
            members[used:used + m] += 0.008 * u
            used += m
            xy.append(c + (0.008 + eps * (1 - 1e-4)) * u), z.append(rng.uniform(-1.5, 0.5)), tag.append(SATELLITE)
        xy.extend(members), z.extend(-2.0 + 0.2 * rng.permutation(30)), tag.extend([POLE] * 30)
    g = 0
    for f in np.arange(0.72, 0.805, 0.01):
        for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            w = f * eps
            i, j = 20 + 9 * g, -150 + 13 * g
            low = np.array([i * w, j * w])
            a = low + np.where(np.array([sx, sy]) > 0, 0.002 * eps, w - 0.002 * eps)
            xy.extend([a] * 5), z.extend(0.2 * np.arange(5)), tag.extend([CORNER_GROUP] * 5)
            xy.append(a + 0.7085 * eps * np.array([sx, sy])), z.append(0.0), tag.append(CORNER_FAR)
            g += 1
    xy, z, tag = np.array(xy), np.array(z), np.array(tag)
    return Scene('poles', eps, *_sprinkle_unselected(rng, xy, z, np.zeros(len(xy), np.int64), tag, 0.05), check=_check_poles)


def _check_poles(v, lab):
    _labels_are_ranks(v, lab)
    a = Analysis(v, 0)
    cells = np.floor(a.kxy / (0.7 * v.eps)).astype(np.int64)
    _, cinv, ccnt = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    dense = ccnt[cinv.ravel()] >= MIN_SAMPLES
    assert dense[a.tag == POLE].mean() > 0.8
    owned = [r for r in np.flatnonzero(a.border) if dense[a.near[r] & a.core].all()]
    assert len(owned) >= 5 and (a.tag[owned] == SATELLITE).sum() >= 5, len(owned)
    sat = a.tag == SATELLITE
    assert a.border[sat].mean() > 0.9 and (a.near[sat].sum(1) < MIN_SAMPLES).mean() > 0.9    # but for one that lands next to another pole
    # poles across a cell boundary: members of one pole in two cells, the smaller part not dense on its own
    assert (a.core & ~dense & (a.tag == POLE)).sum() >= 10
    far = a.tag == CORNER_FAR
    assert far.sum() == 36 and a.noise[far].all() and a.core[a.tag == CORNER_GROUP].all()
    d = np.sqrt(((a.kxy[far][:, None] - a.kxy[None]) ** 2).sum(2))
    d[:, far] = np.inf
    assert (d.min(1) > v.eps).all() and (d.min(1) < 1.01 * v.eps).all()


# ------------------------------------------------------------------------------------------------- 6: voxel rounding ties
TIE, PARTNER, FILL = 1, 2, 3


def exact_halves(voxel, lo, hi):
    """float32 x > 0 whose float32 quotient by float32(voxel) is k + 0.5 exactly, for the integers k in [lo, hi)."""
    v = np.float32(voxel)
    k = np.arange(lo, hi)
    q = (k + 0.5).astype(np.float32)
    x = (q * v).astype(np.float32)
    out = {}
    for c in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(1e9))):
        hit = (c / v).astype(np.float32) == q
        for kk, xx in zip(k[hit], c[hit]):
            out.setdefault(int(kk), np.float32(xx))
    return out


@functools.lru_cache(None)
def _ties_scene(use_offset):
    """Groups of 5 points in 5 voxels in a row, one of them exactly half way between two voxels: T (the tie, between voxels k and
    k + 1), a partner in voxel k or in k + 1, and fill points in k + 2, k + 3, k + 4.  If T rounds into its partner's voxel 4 kept
    points remain (noise), otherwise 5 (one core point in the middle, a cluster).  Both signs, both parities of k, ties along
    x, y and z."""
    voxel = 0.05 if use_offset else 0.15
    v = np.float32(voxel)
    halves = exact_halves(voxel, 20, int(70 / voxel))
    rng = np.random.RandomState(6)
    ks = np.array(sorted(halves))
    pick = np.concatenate([rng.choice(ks[ks % 2 == par], 36, replace=False) for par in (0, 1)])
    xy, z, tag = [], [], []
    for g, k in enumerate(pick):
        k = int(k)
        sign = -1.0 if g % 2 else 1.0
        axis = (g // 2) % 3                                          # the axis along which the group lies (2: ties in z)
        partner = k if (g // 6) % 2 else k + 1
        a = np.array([halves[k]] + [np.float32(j) * v for j in (partner, k + 2, k + 3, k + 4)], np.float32) * np.float32(sign)
        if axis == 2:                                                # same voxel column but for the tie and its partner: T, P | fill
            a_z = np.array([halves[k] * sign, np.float32(partner) * v * sign, 0, 0, 0], np.float32)
            c = np.zeros((5, 3), np.float32)
            c[:, 0] = np.float32(40 * (g % 7 - 3)) * v + np.array([0, 0, 1, 2, 3], np.float32) * v
            c[:, 1] = np.float32(100 * (g - 36) + 7) * v
            c[:, 2] = a_z
        else:
            c = np.zeros((5, 3), np.float32)
            c[:, axis] = a
            c[:, 1 - axis] = np.float32(100 * (g - 36) + 7) * v if axis == 0 else np.float32(60 * (g - 36) + 3) * v
            c[:, 2] = np.float32(g % 5 - 2) * v
        xy.extend(c[:, :2]), z.extend(c[:, 2]), tag.extend([TIE, PARTNER, FILL, FILL, FILL])
    xy, z, tag = np.array(xy, np.float32), np.array(z, np.float32), np.array(tag)
    return Scene('ties_%s' % ('offset' if use_offset else 'plain'), 0.4, xy, z, np.zeros(len(z), np.int64), tag, check=_check_ties)


def _check_ties(v, lab):
    _labels_are_ranks(v, lab)
    src = v.seen()[v.mos == 1]
    tie = v.tag[v.mos == 1] == TIE
    q = (src / np.float32(v.voxel)).astype(np.float32)
    frac = np.abs(q - np.trunc(q))
    assert ((frac == 0.5).any(1) & tie).sum() >= 50                             # the quotient the voxel key rounds is k + 0.5 exactly
    half = q[(frac == 0.5)]
    assert (half > 0).sum() >= 10 and (half < 0).sum() >= 10
    assert (np.floor(np.abs(half)) % 2 == 0).sum() >= 10 and (np.floor(np.abs(half)) % 2 == 1).sum() >= 10
    even, up = kept_voxels(src, v.voxel), kept_voxels(src, v.voxel, round_half_up)
    assert len(even[0]) != len(up[0]) or not np.array_equal(even[1], up[1])      # half-even and half-up keep different sets
    # ... and the labels tell: ties whose group is a cluster only because of the way the tie rounded, and the other way round
    t_lab = lab[v.mos == 1][tie]
    assert (t_lab > 0).sum() >= 10 and (t_lab == 0).sum() >= 10


# ------------------------------------------------------------------------------------------------- 7: far field
def _far_scene():
    rng = np.random.RandomState(7)
    centres = [(74, 74), (-74, 74), (74, -74), (-74, -74)] + [tuple(rng.uniform(-75, 75, 2)) for _ in range(8)] + [(500.0, -500.0)]
    xy, tag = [], []
    for k, c in enumerate(centres):
        n = int(rng.randint(80, 160))
        xy.append(np.array(c) + rng.randn(n, 2) * rng.uniform(0.3, 1.0, 2)), tag.append(np.full(n, k + 1))
    xy, tag = np.concatenate(xy), np.concatenate(tag)
    return Scene('far', 0.4, *_sprinkle_unselected(rng, xy, rng.uniform(-1.5, 0.5, len(xy)), np.zeros(len(xy), np.int64), tag),
                 check=_check_far)


def _check_far(v, lab):
    _labels_are_ranks(v, lab)
    a = Analysis(v, 0)
    assert a.border.sum() >= 100, a.border.sum()
    assert np.abs(a.kxy).max() > 499 and (np.abs(a.kxy[np.abs(a.kxy).max(1) < 100]).max(1) > 74).sum() > 100
    assert lab[v.tag == len(np.unique(v.tag[v.tag > 0]))].max() > 0             # the blob at 500 m is a cluster


# ------------------------------------------------------------------------------------------------- 8: past one grid pass
def big_lattices(shapes, s=0.25):
    """One exact s-lattice per sample, centred on the origin; all points selected."""
    xy, batch, corner = [], [], []
    for b, (nx, ny) in enumerate(shapes):
        p, tag = lattice(nx, ny, s, s, -s * (nx - 1) / 2 - s / 2, -s * (ny - 1) / 2 - s / 2)
        xy.append(p), batch.append(np.full(len(p), b)), corner.append(tag == CORNER)
    xy = np.concatenate(xy)
    z = np.random.RandomState(8).uniform(-1.5, 0.5, len(xy))
    return Scene('big_lattice', s, xy, z, np.concatenate(batch), np.concatenate(corner).astype(np.int64), check=None)


def big_lattice_expected(v):
    """eps = spacing: every sample is one cluster (label 1) but for its four corners (noise, 0); no cluster is small enough to drop."""
    return np.where(v.tag == 1, 0, 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------- 9: samples
N_SAMPLES = 64
GATE_AT, GATE_OVER, EMPTY, UNSELECTED_ONLY = 12, 13, (5, 6, 30), (9, 31)


@functools.lru_cache(None)
def _samples_scene(min_p_cluster):
    """64 samples: tight blobs (clusters), stray points, unselected points; samples without points, samples without a selected point, one
    with exactly min_p_cluster selected points in as many voxels (a cluster large enough to stay, but the gate on the number of selected
    points is a strict >) and one with one more; and selected points whose sample index is
    outside [0, 64), which are ignored."""
    rng = np.random.RandomState(9)
    xy, tag, batch = [], [], []

    def blob(b, n, t):
        xy.append(rng.uniform(-70, 70, 2) + rng.randn(n, 2) * 0.05), tag.append(np.full(n, t)), batch.append(np.full(n, b))

    def patch(b, n):
        # n points 0.16 apart on a 4-wide lattice: no two share a voxel (5 or 15 cm), and from 5 points on they are one cluster
        i = np.arange(n)
        xy.append(rng.uniform(-70, 70, 2) + 0.16 * np.stack([i % 4, i // 4], 1)), tag.append(np.full(n, 1)), batch.append(np.full(n, b))

    blob(-1, 10, 1)                                                              # before the first sample
    for b in range(N_SAMPLES):
        if b in EMPTY:
            continue
        if b in UNSELECTED_ONLY:
            blob(b, 40, UNSEL)
        elif b == GATE_AT:
            patch(b, min_p_cluster)
            blob(b, 7, UNSEL)
        elif b == GATE_OVER:
            patch(b, min_p_cluster + 1)
        else:
            for k in range(int(rng.randint(2, 5))):
                blob(b, int(rng.randint(4, 40)), k + 1)
            blob(b, 5, UNSEL)
            xy.append(rng.uniform(-70, 70, (6, 2))), tag.append(np.full(6, 9)), batch.append(np.full(6, b))   # strays
    blob(N_SAMPLES, 12, 1)
    blob(N_SAMPLES + 6, 12, 1)
    xy, tag, batch = np.concatenate(xy), np.concatenate(tag), np.concatenate(batch)
    return Scene('samples_%d' % min_p_cluster, 0.4, xy, rng.uniform(-1.5, 0.5, len(xy)), batch, tag, n_batches=N_SAMPLES,
                 check=functools.partial(_check_samples, min_p_cluster=min_p_cluster))


def _check_samples(v, lab, min_p_cluster):
    _labels_are_ranks(v, lab)
    b = v.ti[:, 0]
    assert set(range(N_SAMPLES)) - set(b.tolist()) == set(EMPTY) and b.min() < 0 and b.max() >= N_SAMPLES
    for u in UNSELECTED_ONLY:
        assert (b == u).sum() > 0 and v.mos[b == u].sum() == 0
    assert v.mos[b == GATE_AT].sum() == min_p_cluster and v.mos[b == GATE_OVER].sum() == min_p_cluster + 1
    assert lab[b == GATE_AT].max() == 0
    if min_p_cluster >= MIN_SAMPLES:
        assert lab[b == GATE_OVER].max() == 1
    assert v.mos[(b < 0) | (b >= N_SAMPLES)].sum() >= 30 and lab[(b < 0) | (b >= N_SAMPLES)].max() == 0
    assert sum(lab[b == u].max() >= 2 for u in range(N_SAMPLES) if (b == u).any()) >= 20


# ------------------------------------------------------------------------------------------------- the list
_fixed = functools.lru_cache(None)
BUILDERS = {
    'exact_025': _fixed(lambda: _lattice_scene('exact_025', 0.25, 0.25, 0.25, DYADIC, _check_exact)),
    'exact_05': _fixed(lambda: _lattice_scene('exact_05', 0.5, 0.5, 0.5, DYADIC, _check_exact)),
    'exact_345': _fixed(lambda: _lattice_scene('exact_345', 0.625, 0.375, 0.5, DYADIC, _check_345)),
    'straddle_04': _fixed(lambda: _lattice_scene('straddle_04', 0.4, 0.4, 0.4, ((0.0, 0.0, 40, 30), (7.3, -3.9), (-37.3, 21.7)),
                                                    _check_straddle)),
    'straddle_025': _fixed(lambda: _lattice_scene('straddle_025', 0.25, 0.25, 0.25, ((0.07, 13.13), (13.13, 0.07), (0.07, 0.07)),
                                                     _check_straddle)),
    'shared_border': _fixed(_shared_border_scene),
    'spiral1': _fixed(lambda: _spiral_scene(1)),
    'spiral2': _fixed(lambda: _spiral_scene(2)),
    'poles': _fixed(_poles_scene),
    'far': _fixed(_far_scene),
}


def scene(name, use_offset, min_p_cluster):
    if name == 'ties':
        return _ties_scene(bool(use_offset))
    if name == 'samples':
        return _samples_scene(int(min_p_cluster))
    return BUILDERS[name]()
