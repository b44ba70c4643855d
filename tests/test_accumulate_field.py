"""The exact, truncated distance field of a box of voxels of the accumulated scene cloud, its planar form and the lookup of points in it (include/pcacc.h
C19): AccumulatedCloud.distance_field / clearance / inflate.

Every result is an integer, so every claim is an equality of integers; no tolerance appears anywhere.
  CPU   the g++ build of csrc/accum_field.h (tests/accum_field_host_driver.cpp: every index asserted, every output poisoned first and written once, the
        poison behind it intact, every pass run cell by cell, upwards and downwards, and along the contiguous axis again chunk by chunk in a scrambled order) against the brute-force
        restatement over ALL sites of the box (tests/accumulate_field_reference.py: no passes, no packing, no keys); scipy's distance_transform_edt as
        a third witness of dist2; the capability scene (a room with a pillar) on the restatement alone;
  GPU   both entry points against the g++ build on the same cases, identities that tie the grids to extract() and knn(), clearance(), a life cycle, the model forward and the argument checks.
A tie: the rows of extract() ascend in (x, y, z), and every pass walks its window upwards, so among sites at equal d2 the lowest row is also the one a
pass meets first; a rule "the first met wins" and the rule of the contract differ only for a pass that walks downwards.  So the g++ driver walks every
window of every pass downwards as well, where the lowest row is the LAST one met, and asserts the same word; the tie tests state the winner by its
coordinates, on the g++ build, and the restatement decides it without any walk: the first entry of the row-ordered list at the minimum."""
import os

import numpy as np
import pytest
import torch

import accumulate_field_reference as fref
import accumulate_helpers as ah
import accumulate_knn_reference as kref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

RADII = (1, 2, 7, 128)
SHAPES = ((1, 1, 1), (1, 1, 65), (65, 1, 1), (1, 65, 1), (3, 67, 5), (2, 2, 63), (2, 2, 64), (2, 2, 65), (2, 2, 257))
ORIGIN = (-2, 5, -31)                                                               # of the boxes of SHAPES
R5 = ((3, 4, 0), (5, 0, 0), (4, 4, 0), (5, 1, 0))                                   # d2 = 25, 25, 32, 26 at R = 5
R5_PROBES = [(10 + 30 * k, 10, 3) for k in range(4)]
FILTERED = {(0, 0, 0): (2, 0), (2, 0, 0): (1, 0), (3, 1, 0): (2, 2), (7, 0, 0): (3, 0)}    # from (1, 0, 0): nearest (0,0,0) / (2,0,0); min_count 2 drops the latter
PLANAR_COLUMNS = [(1, 1, 2), (1, 1, 5), (4, 2, 9), (3, 3, -1), (5, 0, 8), (5, 0, 9)]    # two in one column; the only voxel just above / below [0, 9); one in, one out


# ---- scenes: a ReferenceMap each, built once and never modified ------------------------------------------------------------------------------------------
def _corners(shape):
    return sorted({(ORIGIN[0] + a * (shape[0] - 1), ORIGIN[1] + b * (shape[1] - 1), ORIGIN[2] + c * (shape[2] - 1)) for a in (0, 1) for b in (0, 1) for c in (0, 1)})


def _every(shape):
    return [(ORIGIN[0] + i, ORIGIN[1] + j, ORIGIN[2] + k) for i in range(shape[0]) for j in range(shape[1]) for k in range(shape[2])]


def _random_voxels(origin, shape, share, seed):
    rs = np.random.RandomState(seed)
    at = np.argwhere(rs.uniform(0, 1, shape) < share)
    return [tuple(int(v) + o for v, o in zip(c, origin)) for c in at]


_scenes = {}


def _build_scene(name):
    if name == 'empty':
        return ref.ReferenceMap(0.1)
    if name == 'elsewhere':                                                         # a map, and no voxel of it in any box of SHAPES
        return ah.rows([(500, 500, 500), (-400, 7, 9)], 2)[0]
    if name.startswith('corners') or name.startswith('every'):
        shape = SHAPES[int(name.split('_')[1])]
        return ah.rows((_corners if name.startswith('corners') else _every)(shape), 11)[0]
    if name == 'tie2':                                                              # (+-3, 0, 0) around (0, 0, 0), and the same along y and z further out
        return ah.rows([(-3, 0, 0), (3, 0, 0), (20, -2, 0), (20, 2, 0), (40, 0, -4), (40, 0, 4)], 12)[0]
    if name == 'tie4':                                                              # four at d2 = 25 from (0, 0, 0), on three different x
        return ah.rows([(0, 5, 0), (3, 4, 0), (4, -3, 0), (5, 0, 0), (-3, 0, 4)], 13)[0]
    if name == 'r5':
        return ah.rows([tuple(p[a] + o[a] for a in range(3)) for p, o in zip(R5_PROBES, R5)], 14)[0]
    if name == 'filtered':
        return ah.records(0.1, FILTERED)
    if name == 'rows343':
        return ah.records(0.1, ah.random_rows(343, 443)[0])
    if name == 'edge':
        vox, decoys = ah.bound_voxels()
        return ah.rows(sorted(set(vox + decoys)), 15, vs=0.01)[0]
    if name == 'random':                                                            # 40 x 33 x 70 at about 1 %
        return ah.rows(_random_voxels((-7, 3, -20), (40, 33, 70), 0.01, 16), 16)[0]
    if name == 'planar_columns':
        return ah.rows(PLANAR_COLUMNS, 19)[0]
    assert name == 'wavy'
    return ah.points_map(0.1, [(ah.wavy(), None, 0)])


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene and the arguments of one field call; each also runs in its planar form ---------------------------------------------------------------
def _cases():
    cases = {}
    for s, shape in enumerate(SHAPES):
        for R in RADII:
            cases['s%d_r%d_empty' % (s, R)] = ('empty' if R == 2 else 'elsewhere', dict(origin=ORIGIN, shape=shape, max_radius=R))     # m = 0, and 0 sites of m = 2
            cases['s%d_r%d_corners' % (s, R)] = ('corners_%d' % s, dict(origin=ORIGIN, shape=shape, max_radius=R))
            cases['s%d_r%d_every' % (s, R)] = ('every_%d' % s, dict(origin=ORIGIN, shape=shape, max_radius=R))
    cases['tie2'] = ('tie2', dict(origin=(-4, -5, -6), shape=(46, 9, 12), max_radius=6))
    cases['tie4'] = ('tie4', dict(origin=(-4, -4, -1), shape=(11, 11, 6), max_radius=6))
    cases['r5'] = ('r5', dict(origin=(5, 8, 2), shape=(105, 8, 3), max_radius=5))
    cases['filtered_all'] = ('filtered', dict(origin=(-1, -1, -1), shape=(10, 4, 3), max_radius=4))
    cases['filtered_min2'] = ('filtered', dict(origin=(-1, -1, -1), shape=(10, 4, 3), max_radius=4, min_count=2))
    cases['filtered_static'] = ('filtered', dict(origin=(-1, -1, -1), shape=(10, 4, 3), max_radius=4, max_moving_fraction=0.5))
    cases['rows343_half_outside'] = ('rows343', dict(origin=(0, 0, 0), shape=(8, 8, 8), max_radius=3))
    cases['rows343_cut'] = ('rows343', dict(origin=(-1, -2, 0), shape=(4, 5, 6), max_radius=7, min_count=2, max_moving_fraction=0.5))
    cases['rows343_beside'] = ('rows343', dict(origin=(6, -3, -3), shape=(5, 7, 7), max_radius=4))      # no site inside: all -1 although voxels lie 3 away
    for axis in range(3):
        for lo in (EDGE - 4, -EDGE - 5):                                            # across 2^20 - 1 and across -2^20
            origin, shape = [-2, -2, -2], [5, 5, 5]
            origin[axis], shape[axis] = lo, 8
            cases['edge_axis%d_%s' % (axis, 'hi' if lo > 0 else 'lo')] = ('edge', dict(origin=tuple(origin), shape=tuple(shape), max_radius=4))
    cases['edge_far'] = ('edge', dict(origin=(1 << 31, -(1 << 31), (1 << 31) - 2), shape=(2, 3, 2), max_radius=128))   # the largest origin: no cell in the grid
    cases['random_r6'] = ('random', dict(origin=(-7, 3, -20), shape=(40, 33, 70), max_radius=6))
    cases['random_r128'] = ('random', dict(origin=(-7, 3, -20), shape=(40, 33, 70), max_radius=128))     # above the diagonal: untruncated
    cases['planar_columns'] = ('planar_columns', dict(origin=(0, 0, 0), shape=(7, 5, 9), max_radius=3))
    for name in list(cases):
        cases[name + '_planar'] = (cases[name][0], dict(cases[name][1], planar=True))
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)
WAVY = {'wavy': ('wavy', dict(origin=(-32, -32, -12), shape=(64, 64, 24), max_radius=8)),
        'wavy_planar': ('wavy', dict(origin=(-32, -32, -12), shape=(64, 64, 24), max_radius=8, planar=True))}
_restated, _hosted = {}, {}


def _args(name):
    scene, a = (CASES.get(name) or WAVY[name])
    return scene, dict(dict(planar=False, min_count=1, max_moving_fraction=None), **a)


def _restate(name):
    if name not in _restated:
        scene, a = _args(name)
        _restated[name] = fref.field(_scene(scene), a['origin'], a['shape'], a['max_radius'], a['planar'], a['min_count'], a['max_moving_fraction'])
    return _restated[name]


POSE = ah.rot_xyz(0.3, -0.2, 0.5, (0.4, -0.3, 0.2))


def _lookup_rows(name):
    """The rows looked up in the field of a case: voxel rows over the box and one cell around it (so: seen, far, outside), rows at and beyond the grid's
    edge; and as points the centres of the same voxels pulled back through POSE, with a NaN and a point beyond 2^20 voxels."""
    scene, a = _args(name)
    (x0, y0, z0), (nx, ny, nz) = a['origin'], a['shape']
    rs = np.random.RandomState(len(name))
    n = 48
    coords = np.stack([rs.randint(x0 - 1, x0 + nx + 1, n), rs.randint(y0 - 1, y0 + ny + 1, n), rs.randint(z0 - 1, z0 + nz + 1, n)], 1)
    coords = np.clip(coords, -(1 << 31), (1 << 31) - 1)
    coords = np.concatenate([coords, [[x0, y0, z0], [x0 + nx - 1, y0 + ny - 1, z0 + nz - 1], [x0 + nx, y0, z0], [x0, y0, z0 - 1], [EDGE, 0, 0], [0, -EDGE - 1, 0],
                                      [EDGE - 1, -EDGE, EDGE - 1], [ah.I32_MAX, 0, ah.I32_MIN]]]).astype(np.int64)
    coords = np.clip(coords, ah.I32_MIN, ah.I32_MAX).astype(np.int32)
    vs = _scene(scene).voxel_size
    inside = np.all(np.abs(coords.astype(np.int64)) < 30000, 1)                     # the rest would not survive float32 and the pose
    world = (coords[inside].astype(np.float64) + 0.5) * vs
    back = np.linalg.inv(POSE)
    pts = (world @ back[:3, :3].T + back[:3, 3]).astype(np.float32)
    pts = np.concatenate([pts, [[np.nan, 0, 0], [0, np.inf, 0], [6.0e4, 0, 0], [0, 0, -6.0e4]]]).astype(np.float32)
    return pts, coords


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_field_host_driver', 'field_host')
LOOKED = [('status', np.uint8), ('dist2', np.int32), ('row', np.int32)]


def _run_host(exe, tmp_path, tag, r, pts, coords, origin, shape, max_radius, planar, min_count, max_moving_fraction, spare=3):
    keys, acc, _ = r.records()
    m = keys.shape[0]
    head = [m, m + spare, min_count, 0 if max_moving_fraction is None else 1, max_radius, 1 if planar else 0] + list(origin) + list(shape) + [len(pts), len(coords)]
    reals = [0.0 if max_moving_fraction is None else max_moving_fraction, r.voxel_size] + POSE.reshape(-1).tolist()
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array(reals, np.float64), ah.map_bytes(keys, acc), np.asarray(pts, np.float32),
                        np.asarray(coords, np.int32))
    grid = (shape[0], shape[1], 1 if planar else shape[2])
    out, off = ah.unpack(raw, 0, [('counters', np.int64, (4,)), ('dist2', np.int32, grid), ('nearest', np.int32, grid)])
    for what, n in (('points', len(pts)), ('coords', len(coords))):
        out[what], off = ah.unpack(raw, off, [('counters', np.int64, (4,))] + [(f, d, (n,)) for f, d in LOOKED])
    assert off == len(raw)
    return out


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, a = _args(name)
        pts, coords = _lookup_rows(name)
        _hosted[name] = _run_host(exe, tmp_path, name, _scene(scene), pts, coords, **a)
    return _hosted[name]


def _built(exe, tmp_path, name):
    """The g++ build's grids and counters of a case, held to the restatement's first."""
    got = _host(exe, tmp_path, name)
    _assert_same_field(got, _restate(name), name)
    return dict(got, counters=got['counters'].tolist())


def _assert_same_field(got, want, what):
    assert [int(v) for v in got['counters']] == [int(v) for v in want['counters']], (what, got['counters'], want['counters'])
    for f in ('dist2', 'nearest'):
        assert got[f].dtype == np.int32 and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def _assert_same_rows(got, want, what):
    assert [int(v) for v in got['counters']] == [int(v) for v in want['counters']], (what, got['counters'], want['counters'])
    for f, d in LOOKED:
        assert got[f].dtype == d and np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:5].tolist())


def _coords_of(r, min_count=1, max_moving_fraction=None):
    return np.array([c for c, _ in fref.cref.kept_rows(r, min_count, max_moving_fraction)], np.int64).reshape(-1, 3)


# ---- CPU: host build == restatement ------------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for(host_exe, tmp_path):
    built = lambda name: _built(host_exe, tmp_path, name)
    assert len(CASE_NAMES) == 2 * (len(SHAPES) * len(RADII) * 3 + 19)
    assert built('s0_r2_empty')['counters'] == [0, 0, 0, 0] and built('s0_r1_empty')['counters'] == [2, 0, 0, 1]          # m = 0; m = 2 and no site
    assert built('s4_r7_corners')['counters'][:2] == [8, 8] and built('s4_r7_corners_planar')['counters'][:2] == [8, 4]
    assert built('s8_r128_every')['counters'] == [1028, 1028, 1028, 0] and built('s8_r128_every_planar')['counters'] == [1028, 4, 4, 0]
    assert built('rows343_beside')['counters'][1:] == [0, 0, 245] and _restate('rows343_half_outside')['voxels'] == 64
    cut = built('rows343_cut')
    assert 0 < cut['counters'][1] < 120 and cut['counters'][0] < 343
    for name in CASE_NAMES:
        if name.startswith('edge_axis') and not name.endswith('_planar'):
            f = built(name)
            assert f['counters'][1] > 0 and f['counters'][3] > 0, name               # sites at the edge of the grid, and cells that see none
    assert built('edge_far')['counters'][1:] == [0, 0, 12]
    assert 800 < built('random_r6')['counters'][1] < 1050 and built('random_r128')['counters'][3] == 0


def test_ties_go_to_the_lowest_row(host_exe, tmp_path):
    built = lambda name: _built(host_exe, tmp_path, name)
    two, origin = built('tie2'), CASES['tie2'][1]['origin']
    rows = [c for c, _ in fref.cref.kept_rows(_scene('tie2'))]
    assert rows == [(-3, 0, 0), (3, 0, 0), (20, -2, 0), (20, 2, 0), (40, 0, -4), (40, 0, 4)]
    for cell, d2, row in (((0, 0, 0), 9, 0), ((20, 0, 0), 4, 2), ((40, 0, 0), 16, 4)):
        at = tuple(c - o for c, o in zip(cell, origin))
        assert (two['dist2'][at], two['nearest'][at]) == (d2, row)
    four, origin = built('tie4'), CASES['tie4'][1]['origin']
    rows = [c for c, _ in fref.cref.kept_rows(_scene('tie4'))]
    assert rows == [(-3, 0, 4), (0, 5, 0), (3, 4, 0), (4, -3, 0), (5, 0, 0)]          # from (0, 0, 0) all five lie at d2 = 25
    at = tuple(-o for o in origin)
    assert (four['dist2'][at], four['nearest'][at]) == (25, 0)
    assert (four['dist2'][at[0], at[1], at[2] - 1], four['nearest'][at[0], at[1], at[2] - 1]) == (26, 1)      # one below: (-3, 0, 4) is 34 away, four tie at 26
    flat = built('tie4_planar')                                                  # in (x, y): (-3, 0) at 9 is alone
    assert (flat['dist2'][at[0], at[1], 0], flat['nearest'][at[0], at[1], 0]) == (9, 0)


def test_the_cut_is_euclidean_not_the_window(host_exe, tmp_path):
    built = lambda name: _built(host_exe, tmp_path, name)
    f, origin = built('r5'), CASES['r5'][1]['origin']
    got = [(int(f['dist2'][tuple(p[a] - origin[a] for a in range(3))]), int(f['nearest'][tuple(p[a] - origin[a] for a in range(3))])) for p in R5_PROBES]
    assert got == [(25, 0), (25, 1), (-1, -1), (-1, -1)]                            # 32 and 26 lie inside the window of every pass, and are none
    flat = built('r5_planar')
    assert [int(flat['dist2'][p[0] - origin[0], p[1] - origin[1], 0]) for p in R5_PROBES] == [25, 25, -1, -1]


def test_the_filter_removes_the_nearest_site(host_exe, tmp_path):
    built = lambda name: _built(host_exe, tmp_path, name)
    origin = CASES['filtered_all'][1]['origin']
    at = tuple(c - o for c, o in zip((1, 0, 0), origin))
    every, some, static = built('filtered_all'), built('filtered_min2'), built('filtered_static')
    assert (every['dist2'][at], every['nearest'][at]) == (1, 0) and every['counters'][:2] == [4, 4]
    at3 = tuple(c - o for c, o in zip((3, 0, 0), origin))
    assert (every['dist2'][at3], every['nearest'][at3]) == (1, 1)                   # (2, 0, 0), row 1, before (3, 1, 0), row 2
    assert (some['dist2'][at3], some['nearest'][at3]) == (1, 1) and some['counters'][:2] == [3, 3]     # (2, 0, 0) is gone: (3, 1, 0) is row 1 now
    assert (static['dist2'][at3], static['nearest'][at3]) == (1, 1) and static['counters'][:2] == [3, 3]   # (3, 1, 0) is gone: row 1 is (2, 0, 0)
    assert _coords_of(_scene('filtered'), 2)[1].tolist() == [3, 1, 0] and _coords_of(_scene('filtered'), 1, 0.5)[1].tolist() == [2, 0, 0]


def test_planar_columns(host_exe, tmp_path):
    built = lambda name: _built(host_exe, tmp_path, name)
    f = built('planar_columns_planar')
    rows = [c for c, _ in fref.cref.kept_rows(_scene('planar_columns'))]
    assert rows == [(1, 1, 2), (1, 1, 5), (3, 3, -1), (4, 2, 9), (5, 0, 8), (5, 0, 9)]
    assert f['counters'][:2] == [6, 2] and _restate('planar_columns_planar')['voxels'] == 3     # columns (1, 1) and (5, 0); (3, 3) and (4, 2) hold nothing in [0, 9)
    assert (f['dist2'][1, 1, 0], f['nearest'][1, 1, 0]) == (0, 0) and (f['dist2'][5, 0, 0], f['nearest'][5, 0, 0]) == (0, 4)
    assert (f['dist2'][4, 2, 0], f['nearest'][4, 2, 0]) == (5, 4) and (f['dist2'][3, 3, 0], f['nearest'][3, 3, 0]) == (8, 0)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    scene, a = _args(name)
    want, got = _restate(name), _host(host_exe, tmp_path, name)
    _assert_same_field(got, want, name)
    c = got['counters'].tolist()
    assert c[2] == int((got['dist2'] >= 0).sum()) and (c[2] + c[3] == got['dist2'].size or _scene(scene).num_voxels == 0)
    assert np.array_equal(got['dist2'] >= 0, got['nearest'] >= 0) and int(got['dist2'].max()) <= a['max_radius'] ** 2
    pts, coords = _lookup_rows(name)
    vs = _scene(scene).voxel_size
    _assert_same_rows(got['points'], fref.lookup(fref.voxels_of_points(pts, POSE, vs), want, a['origin'], a['shape'], a['planar']), (name, 'points'))
    _assert_same_rows(got['coords'], fref.lookup(fref.voxels_of_coords(coords), want, a['origin'], a['shape'], a['planar']), (name, 'coords'))
    assert got['coords']['counters'][1] < len(coords) and got['points']['counters'][1] == len(pts) - 4


def test_lookup_rows_cover_every_status(host_exe, tmp_path):
    seen = set()
    for name in ('random_r6', 'random_r6_planar', 'rows343_beside', 'edge_axis0_hi'):
        got = _host(host_exe, tmp_path, name)
        seen |= set(got['coords']['status'].tolist()) | set(got['points']['status'].tolist())
    assert seen == {0, 1, 3, 7}


# ---- CPU: scipy as a third witness ---------------------------------------------------------------------------------------------------------------------------
def test_scipy_agrees_on_the_squared_distances(host_exe, tmp_path):
    ndimage = pytest.importorskip('scipy.ndimage')
    scene, a = _args('random_r128')
    got = _host(host_exe, tmp_path, 'random_r128')
    coords = _coords_of(_scene(scene))
    occ = np.zeros(a['shape'], bool)
    occ[tuple((coords - np.array(a['origin'])).T)] = True
    assert occ.sum() == coords.shape[0] == got['counters'][1]
    edt = np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.int64)
    assert np.array_equal(edt, got['dist2']) and edt.max() < 128 ** 2
    cells = np.stack(np.meshgrid(*[np.arange(o, o + n) for o, n in zip(a['origin'], a['shape'])], indexing='ij'), -1)
    assert np.array_equal(((cells - coords[got['nearest']]) ** 2).sum(-1), got['dist2'])      # scipy breaks ties its own way: nearest is the restatement's
    flat, got2 = occ.any(2), _host(host_exe, tmp_path, 'random_r128_planar')
    assert np.array_equal(np.rint(ndimage.distance_transform_edt(~flat) ** 2).astype(np.int64), got2['dist2'][:, :, 0])


# ---- CPU: the capability scene, on the restatement alone ---------------------------------------------------------------------------------------------------
def _room():
    """0.1 m voxels.  A room of 60 x 60 voxels inside four walls at x, y = -1 and 60, three voxels tall, with a pillar of 4 x 4 voxels in the middle."""
    walls = {(x, y, z) for z in range(3) for x in range(-1, 61) for y in range(-1, 61) if x in (-1, 60) or y in (-1, 60)}
    pillar = {(x, y, z) for z in range(3) for x in range(28, 32) for y in range(28, 32)}
    return ah.records(0.1, {c: (1, 0) for c in walls | pillar})


def _four_connected(mask):
    """The number of 4-connected components of a 2-D bool mask (a flood fill)."""
    left, n = {tuple(c) for c in np.argwhere(mask).tolist()}, 0
    while left:
        n += 1
        stack = [left.pop()]
        while stack:
            x, y = stack.pop()
            for c in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if c in left:
                    left.remove(c)
                    stack.append(c)
    return n


def test_the_room_has_a_clearance_that_no_neighbour_search_reaches():
    r = _room()
    probe = (14, 14, 1)                                                             # 15 voxels = 1.5 m from the walls at x = -1 and y = -1, farther from all else
    near = kref.knn(r, ah.centres([probe], 0.1), k=1, radius=4)
    assert near['found'].tolist() == [0] and near['rows'].tolist() == [[-1]]          # C16 stops at 4 voxels
    f = fref.field(r, (-1, -1, 0), (62, 62, 3), 40)
    rows = [c for c, _ in fref.cref.kept_rows(r)]
    at = (probe[0] + 1, probe[1] + 1, probe[2])
    assert f['dist2'][at] == 225 and rows[f['nearest'][at]] == (-1, 14, 1)           # exact, and of the two walls at 15 the lower row
    assert f['counters'][3] == 0 and int(f['dist2'].max()) < 40 ** 2
    flat = fref.field(r, (-1, -1, 0), (62, 62, 3), 40, planar=True)
    assert np.array_equal(flat['dist2'][:, :, 0], f['dist2'][:, :, 1])               # every column is full: the plane is any slice
    for radius_m, voxels in ((0.6, 5), (2.9, 28)):
        assert int(np.floor(radius_m / 0.1)) == voxels
    free = ~((flat['dist2'][:, :, 0] >= 0) & (flat['dist2'][:, :, 0] <= 5 ** 2))
    assert free.sum() > 1500 and _four_connected(free) == 1                          # one region,
    assert not free[29:33, 29:33].any() and _four_connected(~free) == 2              # around the pillar: what is not free is the walls' band and the pillar's
    assert not (~((flat['dist2'][:, :, 0] >= 0) & (flat['dist2'][:, :, 0] <= 28 ** 2))).any()      # at 2.9 m nothing is left


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
BAD_FIELD_ARGS = (dict(max_radius=0), dict(max_radius=129), dict(origin=(0, 0), shape=(2, 2, 2)), dict(origin=(0, 0, (1 << 31) + 1), shape=(2, 2, 2)),
                  dict(origin=(0, 0, 0), shape=(2, 2)), dict(origin=(0, 0, 0), shape=(0, 2, 2)), dict(origin=(0, 0, 0), shape=(2, 2, -1)),
                  dict(origin=(0, 0, 0), shape=(1 << 10, 1 << 10, 1 << 9), pad=False), dict(origin=(0, 0, 0), shape=(1 << 10, 1 << 10, 1 << 7), max_radius=128),
                  dict(origin=(0, 0, 0), shape=(1 << 14, (1 << 14) + 1, 5), planar=True, pad=False), dict(origin=(3 - (1 << 31), 0, 0), shape=(2, 2, 2), max_radius=4),
                  dict(min_count=0), dict(max_moving_fraction=float('nan')))


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_field_workspace_bytes', 'pcacc_accum_field', 'pcacc_accum_field_lookup'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C19. ' in header and len(native._PROTOTYPES['pcacc_accum_field']) == 21 and len(native._PROTOTYPES['pcacc_accum_field_lookup']) == 19
    assert len(native._PROTOTYPES['pcacc_accum_field_workspace_bytes']) == 3
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = open(os.path.join(csrc, 'accum_field.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_columns.h"']
    for helper in ('accum_unkey(', 'accc_map_row(', 'accc_column_key(', 'accn_in_range(', 'PCACC_BOUND('):
        assert helper in text, helper
    for sentence in ('A site within Euclidean R is within R on every axis.', 'The distance on the other axes is constant along a line.',
                     'A minimum of minima is the minimum.'):
        assert sentence in text, sentence
    kernels = open(os.path.join(csrc, 'accum_field.hip')).read()
    for called in ('accn_rows_launch(', 'accum_wave_count(', 'accf_site(', 'accf_line_min(', 'accf_pass_cell(', 'accf_cut(', 'accf_lookup(', 'accum_point(',
                   'accf_chunk_span('):
        assert called in kernels, called
    assert 'asm' not in kernels and 'atomic' not in kernels.replace('atomics', '') and 'accum_field.hip' in open(os.path.join(csrc, 'Makefile')).read()
    for name, value in (('FIELD_MAX_RADIUS', 128), ('FIELD_COUNTERS', 4), ('FIELD_N_ROWS', 0), ('FIELD_N_SITES', 1), ('FIELD_N_NEAR', 2), ('FIELD_N_FAR', 3),
                        ('FIELD_VALID', 1), ('FIELD_INSIDE', 2), ('FIELD_NEAR', 4), ('FIELD_LOOKUP_COUNTERS', 4), ('FIELD_LOOKUP_ROWS', 0),
                        ('FIELD_LOOKUP_N_VALID', 1), ('FIELD_LOOKUP_N_INSIDE', 2), ('FIELD_LOOKUP_N_NEAR', 3)):
        assert ('#define PCACC_%s %d\n' % (name, value)) in header and getattr(native, name) == value
    assert native.FIELD_MAX_CELLS == fref.MAX_CELLS == 1 << 28 and (fref.MAX_RADIUS, fref.VALID, fref.INSIDE, fref.NEAR) == (128, 1, 2, 4)
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    for call in (cpu.distance_field, lambda: cpu.inflate(0.3), lambda: cpu.clearance(coords=torch.zeros((2, 3), dtype=torch.int32))):
        with pytest.raises(native.NativeError):
            call()
    for bad in BAD_FIELD_ARGS:
        with pytest.raises(ValueError):                                              # before anything is allocated: a CPU map gets this far
            cpu.distance_field(**bad)
        with pytest.raises(ValueError):
            cpu.inflate(0.3, **bad)
    for bad in (dict(radius_m=-0.1), dict(radius_m=float('nan'))):
        with pytest.raises(ValueError):
            cpu.inflate(**bad)
    with pytest.raises(ValueError):
        cpu.clearance()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
_clouds = {}


def _cloud(scene):
    """A device map per scene, shared: the calls do not modify it (a test below says so)."""
    if scene not in _clouds:
        _clouds[scene] = ah.device_cloud(_scene(scene))
    return _clouds[scene]


def _poisoned(shape, dtype, behind=16):
    """A tensor of `shape` with every byte 0xa5 (accum_host.h's POISON_BYTE) and `behind` more poisoned elements behind it -> (the tensor, the whole buffer)."""
    n = int(np.prod(shape, dtype=np.int64))
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((n + behind) * size,), 0xa5, dtype=torch.uint8, device=DEV)
    return buf[:n * size].view(dtype).reshape(shape), buf


def _behind_intact(buf, shape, dtype):
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return bool((buf[n:] == 0xa5).all())


def _binding(m, a, pts, coords):
    """One call of each binding with every output poisoned first and poison behind it.  -> numpy results as the host driver returns them."""
    from pcaccumulation_amd import native
    m._ensure()
    grid = (a['shape'][0], a['shape'][1], 1 if a['planar'] else a['shape'][2])
    out, bufs = {}, {}
    for f in ('dist2', 'nearest'):
        out[f], bufs[f] = _poisoned(grid, torch.int32)
    counters = torch.full((4,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    res = native.accum_field(m._cur, m.num_voxels, a['min_count'], a['max_moving_fraction'], a['origin'], a['shape'], a['max_radius'], a['planar'], out=out,
                             counters=counters)
    assert all(_behind_intact(bufs[f], grid, torch.int32) for f in bufs) and all(res[f].is_cuda for f in res)
    got = {f: res[f].cpu().numpy() for f in res}
    for what, rows, kw in (('points', pts, dict(points=torch.from_numpy(pts).to(DEV), coords=None, pose=torch.from_numpy(POSE).to(DEV))),
                           ('coords', coords, dict(points=None, coords=torch.from_numpy(coords).to(DEV), pose=None))):
        n = len(rows)
        dtypes = dict(status=torch.uint8, dist2=torch.int32, row=torch.int32)
        lout, lbufs = {}, {}
        for f in dtypes:
            lout[f], lbufs[f] = _poisoned((n,), dtypes[f])
        lres = native.accum_field_lookup(voxel_size=m.voxel_size, origin=a['origin'], shape=a['shape'], planar=a['planar'], dist2=res['dist2'],
                                         nearest=res['nearest'], out=lout, counters=torch.full((4,), 0x5a5a5a5a, dtype=torch.int64, device=DEV), **kw)
        assert all(_behind_intact(lbufs[f], (n,), dtypes[f]) for f in dtypes)
        got[what] = {f: lres[f].cpu().numpy() for f in lres}
    return got


def _same(a, b):
    return all((_same(a[f], b[f]) if isinstance(a[f], dict) else np.array_equal(a[f], b[f])) for f in a)


def _assert_binding_equals_host(host, name, m):
    scene, a = _args(name)
    pts, coords = _lookup_rows(name)
    snap = ah.snapshot(m, whole_sidecar=True)
    got = _binding(m, a, pts, coords)
    _assert_same_field(got, host, name)
    _assert_same_rows(got['points'], host['points'], (name, 'points'))
    _assert_same_rows(got['coords'], host['coords'], (name, 'coords'))
    assert _same(got, _binding(m, a, pts, coords)), name                             # a second run gives the same bits
    ah.assert_unchanged(m, snap, name)                                               # read-only: keys, records, stamps, state words, num_voxels
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernels_equal_the_host_build_gpu(host_exe, tmp_path, name):
    scene, a = _args(name)
    m = _cloud(scene)
    got = _assert_binding_equals_host(_host(host_exe, tmp_path, name), name, m)
    f = m.distance_field(a['origin'], a['shape'], a['max_radius'], a['planar'], False, a['min_count'], a['max_moving_fraction'])      # the method: the same call
    assert np.array_equal(f['dist2'].cpu().numpy(), got['dist2']) and np.array_equal(f['nearest'].cpu().numpy(), got['nearest'])
    assert f['counters'].tolist() == got['counters'].tolist() and (f['origin'], f['shape'], f['planar']) == (a['origin'], a['shape'], a['planar'])
    want = np.where(got['dist2'] >= 0, np.sqrt(np.maximum(got['dist2'], 0).astype(np.float64)) * m.voxel_size, np.inf).astype(np.float32)
    assert f['distance'].dtype == torch.float32 and np.array_equal(ah.bits(f['distance'].cpu().numpy()), ah.bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(WAVY))
def test_a_map_of_more_than_one_scan_chunk_gpu(host_exe, tmp_path, name):
    """76 661 voxels, a 64 x 64 x 24 box at R = 8: the row table runs over several chunks, the passes over many workgroups."""
    got = _assert_binding_equals_host(_host(host_exe, tmp_path, name), name, _cloud('wavy'))
    assert got['counters'][0] == 76661 and 4000 < got['counters'][1] <= got['counters'][2]           # every column of the sheet holds a voxel: 4096 planar sites


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['random_r6', 'rows343_cut', 'rows343_half_outside', 'planar_columns_planar', 'random_r6_planar'])
def test_the_grids_agree_with_extract_gpu(name):
    scene, a = _args(name)
    m = _cloud(scene)
    filt = dict(min_count=a['min_count'], max_moving_fraction=a['max_moving_fraction'])
    e = m.extract(**filt)['coords'].cpu().numpy().astype(np.int64)
    f = m.distance_field(a['origin'], a['shape'], a['max_radius'], a['planar'], pad=False, **filt)
    dist2, nearest, c = f['dist2'].cpu().numpy(), f['nearest'].cpu().numpy(), f['counters'].tolist()
    axes = 2 if a['planar'] else 3
    lo, n = np.array(a['origin']), np.array(a['shape'])
    inside = np.all((e >= lo) & (e < lo + n), 1)
    at = e[inside] - lo
    if a['planar']:
        at[:, 2] = 0
    zero = np.zeros(dist2.shape, bool)
    zero[tuple(at.T)] = True
    assert np.array_equal(dist2 == 0, zero)                                          # 0 exactly at the kept voxels of the box
    if not a['planar']:
        assert np.array_equal(nearest[tuple(at.T)], np.flatnonzero(inside))          # and nearest there is the row's own number
    cells = np.stack(np.meshgrid(*[np.arange(lo[k], lo[k] + dist2.shape[k]) for k in range(3)], indexing='ij'), -1)
    has = dist2 >= 0
    assert np.array_equal((((cells - e[np.maximum(nearest, 0)])[..., :axes]) ** 2).sum(-1)[has], dist2[has])
    assert c[0] == e.shape[0] and c[1] == int(zero.sum()) and c[2] == int(has.sum()) and c[2] + c[3] == dist2.size
    R = a['max_radius']                                                              # pad=True on the box == the inner slice of pad=False on the grown box
    padded = m.distance_field(a['origin'], a['shape'], R, a['planar'], pad=True, **filt)
    g = (R, R, 0 if a['planar'] else R)
    grown = m.distance_field(tuple(lo - g), tuple(n + 2 * np.array(g)), R, a['planar'], pad=False, **filt)
    inner = tuple(slice(g[k], g[k] + dist2.shape[k]) for k in range(3))
    assert torch.equal(padded['dist2'], grown['dist2'][inner]) and torch.equal(padded['nearest'], grown['nearest'][inner]) and padded['dist2'].is_contiguous()
    assert padded['counters'].tolist() == grown['counters'].tolist() and padded['shape'] == a['shape'] and padded['origin'] == a['origin']
    box = m.distance_field(max_radius=R, planar=a['planar'], pad=False, **filt)      # None: the bounding box of the kept voxels
    if e.shape[0]:
        assert box['origin'] == tuple(e.min(0).tolist()) and box['shape'] == tuple((e.max(0) - e.min(0) + 1).tolist())
        assert box['counters'].tolist()[1] == (len({tuple(c[:2]) for c in e.tolist()}) if a['planar'] else e.shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize('R', [1, 2, 3, 4])
def test_a_small_field_agrees_with_knn_gpu(R):
    """A map whose centroids ARE the voxel centres, queried at voxel centres: the field says `something within R voxels` where knn(k=1) finds a centroid.
    knn compares float64 distances between fixed-point centroids (each up to 2^-17 m off its centre) with max_distance, so a pair at exactly R voxels
    may fall on either side of max_distance = R voxel_size.  For R <= 3 the search runs at radius R + 1 with max_distance = sqrt(R^2 + 1/2) voxels --
    between two integers d2, out of reach of that error -- and must agree at every cell; at R = 4, the largest radius C16 has, it runs at radius 4 with
    its default max_distance and must agree at every cell whose nearest voxel does not lie at exactly 4 voxels (a field at R = 5 says which)."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    vox = _random_voxels((-6, -6, -6), (12, 12, 12), 0.01, 30 + R)
    m = AccumulatedCloud(0.1, DEV, 64)
    m.add(torch.from_numpy(ah.centres(vox, 0.1)).to(DEV))
    f = m.distance_field((-8, -8, -8), (16, 16, 16), R, pad=False)
    cells = np.stack(np.meshgrid(*[np.arange(-8, 8)] * 3, indexing='ij'), -1).reshape(-1, 3)
    points = torch.from_numpy(ah.centres(cells, 0.1)).to(DEV)
    if R < 4:
        near = m.knn(points, 1, radius=R + 1, max_distance=float(np.sqrt(R * R + 0.5)) * 0.1)
        sure = np.ones((16, 16, 16), bool)
    else:
        near = m.knn(points, 1, radius=4)
        sure = m.distance_field((-8, -8, -8), (16, 16, 16), 5, pad=False)['dist2'].cpu().numpy() != 16
    found = near['found'].cpu().numpy().reshape(16, 16, 16) > 0
    assert np.array_equal(found[sure], (f['dist2'].cpu().numpy() >= 0)[sure]) and 0 < found.sum() < found.size and sure.sum() > 0.9 * sure.size
    found &= sure
    rows = near['rows'].cpu().numpy().reshape(16, 16, 16)
    e = m.extract()['coords'].cpu().numpy().astype(np.int64)
    d2 = ((cells.reshape(16, 16, 16, 3) - e[np.maximum(rows, 0)]) ** 2).sum(-1)
    assert np.array_equal(d2[found], f['dist2'].cpu().numpy()[found])                # the same distance; the row may differ among ties (C16 orders by float d2)


@pytest.mark.gpu
def test_clearance_gpu():
    from pcaccumulation_amd import native
    scene, a = _args('random_r6')
    m, r = _cloud(scene), _scene(scene)
    want_field = _restate('random_r6')
    f = m.distance_field(a['origin'], a['shape'], a['max_radius'], pad=False)
    pts, coords = _lookup_rows('random_r6')
    for kw, voxels in ((dict(points=torch.from_numpy(pts).to(DEV), pose=POSE), fref.voxels_of_points(pts, POSE, r.voxel_size)),
                       (dict(coords=torch.from_numpy(coords).to(DEV)), fref.voxels_of_coords(coords)),
                       (dict(coords=torch.from_numpy(coords.astype(np.int64) * (1 << 12)).to(DEV)), fref.voxels_of_coords(coords.astype(np.int64) * (1 << 12)))):
        want = fref.lookup(voxels, want_field, a['origin'], a['shape'])
        got = m.clearance(field=f, **kw)
        _assert_same_rows({k: v.cpu().numpy() for k, v in got.items()}, want, sorted(kw))
        metres = np.where(want['dist2'] >= 0, np.sqrt(np.maximum(want['dist2'], 0).astype(np.float64)) * 0.1, np.inf).astype(np.float32)
        assert np.array_equal(ah.bits(got['distance'].cpu().numpy()), ah.bits(metres))
    status = m.clearance(coords=torch.from_numpy(coords).to(DEV), field=f)['status'].cpu().numpy()
    assert {0, native.FIELD_VALID, native.FIELD_VALID | native.FIELD_INSIDE, native.FIELD_VALID | native.FIELD_INSIDE | native.FIELD_NEAR} == set(status.tolist())
    own = m.clearance(coords=torch.from_numpy(coords).to(DEV), origin=a['origin'], shape=a['shape'], max_radius=a['max_radius'], pad=False)   # its own field
    assert np.array_equal(own['status'].cpu().numpy(), status)
    flat = m.distance_field(a['origin'], a['shape'], a['max_radius'], planar=True, pad=False)
    got = m.clearance(coords=torch.from_numpy(coords).to(DEV), field=flat)
    _assert_same_rows({k: v.cpu().numpy() for k, v in got.items()}, fref.lookup(fref.voxels_of_coords(coords), _restate('random_r6_planar'), a['origin'], a['shape'], True),
                      'planar')
    none = m.clearance(points=torch.zeros((0, 3), device=DEV), field=f)              # n = 0: zero counters, nothing else
    assert none['counters'].tolist() == [0, 0, 0, 0] and none['status'].shape == (0,) and none['distance'].shape == (0,)
    inflated = m.inflate(0.25, field=f)
    assert inflated.dtype == torch.bool and np.array_equal(inflated.cpu().numpy(), (want_field['dist2'] >= 0) & (want_field['dist2'] <= 4))
    assert torch.equal(m.inflate(0.25, origin=a['origin'], shape=a['shape'], max_radius=6, pad=False), inflated)


def _assert_equals_restatement(m, r, what, **kw):
    keys, acc, stamps = m.records()
    mine = r.records()
    assert np.array_equal(keys, mine[0]) and np.array_equal(acc.reshape(5, -1), mine[1])
    e = _coords_of(r, kw.get('min_count', 1), kw.get('max_moving_fraction'))
    origin, shape = (tuple(e.min(0).tolist()), tuple((e.max(0) - e.min(0) + 1).tolist())) if e.shape[0] else ((0, 0, 0), (1, 1, 1))
    got = m.distance_field(pad=False, **kw)
    assert (got['origin'], got['shape']) == (origin, shape), what
    want = fref.field(r, origin, shape, kw.get('max_radius', 32), kw.get('planar', False), kw.get('min_count', 1), kw.get('max_moving_fraction'))
    _assert_same_field({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}, want, what)
    return got


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    import accumulate_prune_reference as rref
    m, r = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1)
    assert m.distance_field()['counters'].tolist() == [0, 0, 0, 0] and m.distance_field()['dist2'].tolist() == [[[-1]]]      # empty: (0, 0, 0) / (1, 1, 1)
    floor = ah.centres([(x, y, (x + y) // 3) for x in range(4, 10) for y in range(-3, 3)], 0.1)
    post = ah.centres([(6, 0, z) for z in range(4, 12)] + [(7, -1, z) for z in (5, 6)], 0.1)

    def both_add(pts, stamp):
        m.add(torch.from_numpy(pts).to(DEV), None, stamp=stamp)
        r.add(pts, None, stamp=stamp)
    both_add(np.concatenate([floor, floor[::2], post]), 0)
    a = _assert_equals_restatement(m, r, 'after add', max_radius=3, min_count=2)
    both_add(np.concatenate([floor[::3], ah.centres([(9, 1, 14), (6, 0, 20)], 0.1)]), 3)
    assert m.prune(before_stamp=2)['kept'] == rref.prune(r, None, before_stamp=2)[0] > 0      # what stamp 3 did not touch goes
    b = _assert_equals_restatement(m, r, 'after prune', max_radius=5)
    assert b['counters'].tolist() != a['counters'].tolist()
    both_add(ah.centres([(-9, 0, 0), (6, 0, 0), (6, 0, 1), (6, 9, 9)], 0.1), 4)
    c = _assert_equals_restatement(m, r, 'add after prune', max_radius=128, planar=True)
    path = os.path.join(str(tmp_path), 'map.npz')
    m.save(path)
    d = _assert_equals_restatement(AccumulatedCloud.load(path, DEV), r, 'after load', max_radius=128, planar=True)
    assert torch.equal(c['dist2'], d['dist2']) and torch.equal(c['nearest'], d['nearest']) and c['counters'].tolist() == d['counters'].tolist()


@pytest.mark.gpu
def test_distance_field_on_the_model_forward_gpu(golden):
    """add_results on the model_tiny_test forward, then distance_field(): it runs and the counters are consistent.  Nothing more is claimed."""
    from helpers import make_batch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    from pcaccumulation_amd.motionnet import MotionNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    dev = torch.device(DEV)
    g = golden('model_tiny_test')
    cfg = default_config('waymo', 'test', n_sweeps=3, xy_range=8)
    inp = make_batch(cfg, [int(s) for s in g['seeds']], int(g['n_frames']), int(g['pts_per_frame']))
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in zip(g['tweak_keys'], g['tweak_vals']):
            sd[str(k)] += torch.from_numpy(v)
        sd['motionhead.mos_seg.seg_head.3.bias'] += torch.tensor([0.0, float(g['mos_shift'])])
    model = model.to(dev).eval().channels_last_()
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
    m = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, stamp=0)
    f = m.distance_field(max_radius=8, pad=False)
    V = m.extract()['points'].shape[0]
    c = f['counters'].tolist()
    assert V == m.num_voxels > 0 and c[0] == c[1] == V == int((f['dist2'] == 0).sum()) and c[2] == int((f['dist2'] >= 0).sum()) and c[2] + c[3] == f['dist2'].numel()
    flat = m.distance_field(max_radius=8, planar=True)
    assert tuple(flat['dist2'].shape) == (f['shape'][0], f['shape'][1], 1) and int((flat['dist2'] == 0).sum()) == flat['counters'].tolist()[1] <= V


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    m = ah.device_cloud(_scene('rows343'))
    snap = ah.snapshot(m, whole_sidecar=True)
    dist2, nearest = (torch.full((4, 5, 6), 7, dtype=torch.int32, device=DEV) for _ in range(2))
    counters = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    rows = {f: torch.full((9,), 7, dtype=d, device=DEV) for f, d in (('status', torch.uint8), ('dist2', torch.int32), ('row', torch.int32))}
    lcounters = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    good = dict(tables=m._cur, m=343, min_count=1, max_moving_fraction=None, origin=(-1, -2, 0), shape=(4, 5, 6), max_radius=3, planar=False,
                out=dict(dist2=dist2, nearest=nearest), counters=counters)
    for bad in (dict(max_radius=0), dict(max_radius=129), dict(origin=((1 << 31) + 1, 0, 0)), dict(m=-1), dict(m=m.capacity + 1)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_field(**dict(good, **bad))
    lib = native.lib()
    keys, acc = native._dev(m._cur[0]), native._dev(m._cur[1])
    field = m.distance_field((-1, -2, 0), (4, 5, 6), 3, pad=False)
    pts = torch.zeros((9, 3), dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    P = native._dev

    def call(keys=keys, acc=acc, cap=m.capacity, rows=343, box=(-1, -2, 0, 4, 5, 6), R=3, planar=0, d=P(dist2), n=P(nearest), cnt=P(counters), ws=P(ws), ws_bytes=ws.numel()):
        return lib.pcacc_accum_field(keys, acc, cap, rows, 1, 0, 0.0, *box, R, planar, d, n, cnt, ws, ws_bytes, native._stream())

    def look(points=P(pts), coords=None, n=9, pose=None, vs=0.1, box=(-1, -2, 0, 4, 5, 6), planar=0, d=P(field['dist2']), nr=P(field['nearest']), s=P(rows['status']),
             od=P(rows['dist2']), orow=P(rows['row']), cnt=P(lcounters)):
        return lib.pcacc_accum_field_lookup(points, coords, n, pose, vs, *box, planar, d, nr, s, od, orow, cnt, native._stream())
    assert call(rows=-1) == call(rows=m.capacity + 1) == call(cap=(1 << 30) + 1) == call(R=0) == call(R=129) == call(R=-1) == -1
    assert call(keys=None) == call(acc=None) == call(d=None) == call(n=None) == call(cnt=None) == call(ws=None) == call(ws_bytes=16) == -1
    big = 1 << 31
    for box in ((big + 1, 0, 0, 4, 5, 6), (0, -big - 1, 0, 4, 5, 6), (0, 0, big + 1, 4, 5, 6), (0, 0, 0, 0, 5, 6), (0, 0, 0, 4, -1, 6), (0, 0, 0, 4, 5, 0),
                (0, 0, 0, 1 << 10, 1 << 10, (1 << 8) + 1), (0, 0, 0, 1 << 40, 1 << 40, 1 << 40), (0, 0, 0, (1 << 28) + 1, 1, 1)):
        assert call(box=box) == look(box=box) == -1, box
    assert call(box=(0, 0, 0, 1 << 14, (1 << 14) + 1, 2), planar=1) == -1
    inside = [native.ctypes.c_void_p(m._cur[0].data_ptr() + 8), native.ctypes.c_void_p(m._cur[1].data_ptr() + 8 * m.capacity)]
    for p in inside:                                                                 # an output that shares bytes with the keys or the records
        assert call(d=p) == call(n=p) == call(cnt=p) == -1
    assert call(n=P(dist2)) == call(d=native.ctypes.c_void_p(nearest.data_ptr() + 4)) == call(cnt=native.ctypes.c_void_p(dist2.data_ptr() + 8)) == -1    # or with another
    need = native.ctypes.c_size_t(0)
    wsb = lib.pcacc_accum_field_workspace_bytes
    assert wsb(-1, 120, native.ctypes.byref(need)) == wsb(343, 0, native.ctypes.byref(need)) == wsb(343, (1 << 28) + 1, native.ctypes.byref(need)) == wsb(343, 120, None) == -1
    assert wsb(343, 120, native.ctypes.byref(need)) == 0 and need.value >= 2 * 8 * 120
    assert look(n=-1) == look(n=(1 << 30) + 1) == look(vs=0.0) == look(vs=float('nan')) == look(vs=float('inf')) == look(cnt=None) == look(d=None) == look(nr=None) == -1
    assert look(points=None) == look(coords=P(torch.zeros((9, 3), dtype=torch.int32, device=DEV))) == look(s=None) == look(od=None) == look(orow=None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in [dist2, nearest, counters, lcounters] + list(rows.values()))      # nothing was launched: the poison stands
    ah.assert_unchanged(m, snap, 'bad arguments')
    for bad in BAD_FIELD_ARGS:
        with pytest.raises(ValueError):
            m.distance_field(**bad)
    for bad in (dict(), dict(points=pts, coords=pts.int()), dict(points=pts[:, :2]), dict(coords=pts), dict(points=pts, field=field, max_radius=3)):
        with pytest.raises(ValueError):
            m.clearance(**bad)
    with pytest.raises(native.NativeError):
        m.clearance(points=pts.cpu(), field=field)
    with pytest.raises(ValueError):
        m.inflate(0.45, field=field)                                                 # 4 voxels against a field of 3
    for bad in (dict(radius_m=3.35), dict(radius_m=0.55, max_radius=4)):             # and against the field it computes itself
        with pytest.raises(ValueError):
            m.inflate(**bad)
    assert call() == 0 and counters.tolist()[0] == 343 and counters.tolist()[2] + counters.tolist()[3] == 120 and not bool((dist2 == 7).any())
    assert torch.equal(dist2, field['dist2']) and torch.equal(nearest, field['nearest'])
    assert look() == 0 and lcounters.tolist() == [9, 9, 9, 9] and rows['status'].tolist() == [7] * 9        # (0, 0, 0) is a voxel of the map: all three bits
    assert rows['dist2'].tolist() == [0] * 9 and len(set(rows['row'].tolist())) == 1 and rows['row'].tolist()[0] >= 0
    assert look(n=0, points=None, s=None, od=None, orow=None) == 0 and lcounters.tolist() == [0, 0, 0, 0]
    empty = native.accum_field(**dict(good, m=0))                                    # m = 0: all -1 and zero counters
    assert empty['counters'].tolist() == [0, 0, 0, 0] and bool((empty['dist2'] == -1).all()) and bool((empty['nearest'] == -1).all())
    ah.assert_unchanged(m, snap, 'after all')
