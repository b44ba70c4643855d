"""Casting rays into the accumulated scene cloud (include/pcacc.h C10): AccumulatedCloud.raycast / raycast_results /
render_range_image.

Every result is an integer, a copied value or a float64 computed by + - * / and sqrt in one order, so every claim is an equality of bits:
  CPU   the g++ build of csrc/accum_raycast.h (tests/accum_raycast_host_driver.cpp, every table index asserted, poison behind the rows in use and in
        every output, every output row written once) against the plain-Python restatement on coordinate dicts (tests/accumulate_raycast_reference.py);
        the restatement against the geometry of the ray (band 1e-9 m, C7's) and against the bound on depth - range_in (slack 1e-9 m);
  GPU   the kernel against the g++ build on the same scenes, then identities that tie raycast to extract and see_through, occlusion and the
        new-object / seen-through / consistent classes on a wall scene, the range image, a life cycle and the model forward.
No test asserts a time."""
import math
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_pierce_reference as pref
import accumulate_prune_reference as rref
import accumulate_query_reference as qref
import accumulate_raycast_reference as yref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

NAN, INF = float('nan'), float('inf')
MISS, HIT, TRUNCATED, SKIPPED, DROPPED = yref.MISS, yref.HIT, yref.TRUNCATED, yref.SKIPPED, yref.DROPPED
EPS = 1e-9                                                                        # C7's band, and the slack of the depth bound


def _bound_on_depth(vs):
    return math.sqrt(3.0) * vs + 2.0 ** -17 + EPS


# ---- scenes: a ReferenceMap, built once and never modified -----------------------------------------------------------------------------------------
def _random_rows(m, seed):
    """m voxels of the 7^3 block around the origin with random records (the random block of the C8 / C9 tests)."""
    rs = np.random.RandomState(seed)
    cells = [(x, y, z) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)]
    rows = {}
    for i in rs.permutation(len(cells))[:m]:
        count = int(rs.randint(1, 7))
        rows[cells[i]] = (count, int(rs.randint(0, count + 1)))
    return rows


# (voxel, points, moving): 1 of 4 sits exactly on 0.25; 1 of 3 and 2 of 4 above; 0 of 2 and 0 of 1 below; 4 of 4   (RATIO_SPEC of the C9 tests)
RATIO_SPEC = [((2, 0, 0), 4, 1), ((-1, 3, 0), 3, 1), ((0, 0, 5), 4, 2), ((0, -2, 1), 2, 0), ((-7, 0, 0), 1, 0), ((2, 0, -1), 4, 4), ((0, 0, -5), 8, 2)]
RATIO_FILTERS = ((dict(min_count=1), 7), (dict(min_count=4), 4), (dict(min_count=5), 1), (dict(min_count=9), 0), (dict(max_moving_fraction=0.25), 4),
                 (dict(max_moving_fraction=float(np.nextafter(0.25, 0))), 2), (dict(max_moving_fraction=0.0), 2),
                 (dict(min_count=3, max_moving_fraction=1.0 / 3.0), 3), (dict(min_count=4, max_moving_fraction=0.25), 2),
                 (dict(max_moving_fraction=1.0), 7))


POSE = ah.rot_xyz(np.deg2rad(4.0), np.deg2rad(-3.0), np.deg2rad(17.0), (0.02, -0.015, 0.017))
SENSOR = np.array([[0.03, 0.02, 0.01]])                                             # the fixed sensor of section 9f
WALL_YZ = [(y, z) for y in range(-20, 20) for z in range(-10, 10)]
GHOST = [(10 + a, 6 + b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]       # held by the map, 2 m in front of the wall
FRESH = [(10 + a, -7 + b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]      # in the scan only, 2 m in front of the wall

_scenes = {}


def _build_scene(name):
    if name.startswith('rows'):
        return ah.records(0.1, _random_rows(int(name[4:]), 100 + int(name[4:])))
    if name == 'third':                                                            # a random third of the 40^3 block around the origin (C7's)
        keep = np.random.RandomState(5).uniform(0, 1, 64000) < 1.0 / 3.0
        return ah.points_map(0.1, [(ah.centres(ah.block(-20, 20)[keep], 0.1), None, 0)])
    if name == 'sparse':                                                           # 2 % of a 40^3 block at 0.25 m
        keep = np.random.RandomState(6).uniform(0, 1, 64000) < 0.02
        return ah.records(0.25, {tuple(c): (1, 0) for c in ah.block(-20, 20)[keep].tolist()})
    if name == 'tie':                                                              # 0.25 is exact; only the last voxel of the written-down walk
        return ah.records(0.25, {(3, 3, 3): (1, 0)})
    if name == 'face':
        return ah.records(0.25, {(-1, 1, 1): (1, 0), (-3, 1, 1): (1, 0)})
    if name == 'face_next':                                                        # the voxel the ray enters at t = -0.0
        return ah.records(0.25, {(1, 1, 1): (1, 0)})
    if name == 'posts':                                                            # three voxels on the x axis at 0.25 m: every number of the ray is exact
        return ah.records(0.25, {(2, 0, 0): (1, 0), (4, 0, 0): (1, 0), (6, 0, 0): (1, 0)})
    if name == 'ratio':
        return ah.records(1.0, {v: (k, j) for v, k, j in RATIO_SPEC})
    if name == 'filter':                                                           # along +x: (0,0,0) 1 of 3 moving, (1,0,0) 2 points, (3,0,0) 5 points
        return ah.records(0.1, {(0, 0, 0): (3, 1), (1, 0, 0): (2, 0), (3, 0, 0): (5, 0), (20, 20, 20): (1, 0)})
    if name == 'bound':
        walked, decoys = ah.walked_voxels()
        return ah.points_map(0.01, [(ah.centres(walked + decoys, 0.01), None, 0)])
    if name == 'walls':                                                            # section 9f's wall, built once (count 1), a second wall 1 m behind it
        rows = {(30, y, z): (1, 0) for y, z in WALL_YZ}
        rows.update({(40, y, z): (2, 0) for y, z in WALL_YZ})
        return ah.records(0.1, rows)
    if name == 'ghost':                                                            # the wall and a cluster the map still holds in front of it
        rows = {(30, y, z): (1, 0) for y, z in WALL_YZ}
        rows.update({v: (1, 0) for v in GHOST})
        return ah.records(0.1, rows)
    assert name == 'wavy'
    return ah.points_map(0.1, [(ah.wavy(), None, 0)])


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene and the arguments of ONE raycast call -------------------------------------------------------------------------------------------
RAY_COUNTS = (0, 1, 63, 64, 65, 257)


def _block_rays(n, seed):
    """n rays around the 7^3 block: three origins inside and beside it, targets over the block and a few voxels beyond."""
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.6, 0.7, (n, 3)).astype(np.float32), rs.uniform(-0.45, 0.55, (3, 3)), rs.randint(0, 3, n).astype(np.int32)


def _bound_rays():
    """Rays that start two voxels inside and point outwards through the LAST voxel of each axis at both ends; two more targets lie outside the grid."""
    ends, starts = [], []
    for axis in range(3):
        for lo, last in ((-EDGE, -EDGE), (EDGE - 3, EDGE - 1)):
            s, e = [1, -2], [1, -2]
            s.insert(axis, lo + (2 if last < 0 else 0))
            e.insert(axis, last)
            starts.append(s)
            ends.append(e)
    outside = np.array([[10485.77, 0.015, -0.015], [0.015, 0.015, -10485.78]], np.float32)
    return (np.concatenate([ah.centres(ends, 0.01), outside]), ah.centres(starts, 0.01).astype(np.float64), np.array([0, 1, 2, 3, 4, 5, 0, 5], np.int32), ends)


def _scan_of_the_ghost_scene():
    """A new scan from SENSOR: every wall voxel's centre (jittered by 0.03 m), then the 27 centres of FRESH."""
    rs = np.random.RandomState(8)
    wall = ah.centres([(30, y, z) for y, z in WALL_YZ], 0.1) + rs.uniform(-0.03, 0.03, (len(WALL_YZ), 3)).astype(np.float32)
    return np.concatenate([wall, ah.centres(FRESH, 0.1)]).astype(np.float32)


POST_O = np.array([[0.125, 0.125, 0.125]])
POST_T = np.array([[2.125, 0.125, 0.125]], np.float32)                            # d = (2, 0, 0), L = 2: voxel k is entered at t = (0.25 k - 0.125) / 2
UP = lambda v: float(np.nextafter(v, np.inf))


def _cases():
    c = {}
    for n in RAY_COUNTS:                                                           # sizes around the wave, against m = 0, 1, 65, 343, under a pose
        for m in (0, 1, 65, 343):
            pts, org, idx = _block_rays(n, 10 * n + m)
            c['n%d_rows%d' % (n, m)] = ('rows%d' % m, pts, org, dict(origin_index=idx, pose=POSE, max_range=0.9))
    pts, org, idx = _block_rays(257, 5)
    c['rows343_to_target'] = ('rows343', pts, org, dict(origin_index=idx, pose=POSE))
    c['rows343_filtered'] = ('rows343', pts, org, dict(origin_index=idx, max_range=1.2, min_range=0.15, min_count=2, max_moving_fraction=0.5))
    pts, org, idx = ah.random_rays()
    c['random'] = ('third', pts, org, dict(origin_index=idx, margin=0.2))
    c['random_range'] = ('third', pts, org, dict(origin_index=idx, max_range=1.5, min_range=0.35))
    # exact ties: every t_a equal at every step; a face start with a negative direction (t = -0.0 steps at once)
    c['ties'] = ('tie', np.array([[1, 1, 1]], np.float32), np.zeros((1, 3)), dict())
    f = float(np.float32(0.3))
    c['face'] = ('face', np.array([[-0.6, 0.3, 0.3]], np.float32), np.array([[0.5, f, f]]), dict())
    c['face_next'] = ('face_next', np.array([[-0.6, 0.3, 0.3]], np.float32), np.array([[0.5, f, f]]), dict())
    # the posts: min_range, max_range, margin and max_steps at their exact boundaries
    c['inside'] = ('posts', POST_T, np.array([[0.625, 0.125, 0.125]]), dict())
    c['plain'] = ('posts', POST_T, POST_O, dict())
    c['min_range_on'] = ('posts', POST_T, POST_O, dict(min_range=0.375))                       # t_start == t_in of voxel 2: the hit
    c['min_range_above'] = ('posts', POST_T, POST_O, dict(min_range=UP(0.375)))                # the next kept voxel
    c['min_range_above_last'] = ('posts', POST_T, POST_O, dict(min_range=UP(1.375)))           # a miss
    c['max_range_on'] = ('posts', POST_T, POST_O, dict(max_range=0.375))                       # t_end == t_in of voxel 2: a miss by the strict <
    c['max_range_above'] = ('posts', POST_T, POST_O, dict(max_range=UP(0.375)))
    c['max_range_past_target'] = ('posts', np.array([[0.25, 0.125, 0.125]], np.float32), POST_O, dict(max_range=1.0))   # the ray runs past its target
    c['max_range_zero'] = ('posts', POST_T, POST_O, dict(max_range=0.0))
    c['margin_L'] = ('posts', POST_T, POST_O, dict(margin=2.0))                                # t_end = 0
    c['margin_above_L'] = ('posts', POST_T, POST_O, dict(margin=2.5))
    c['margin_in_front'] = ('posts', POST_T, POST_O, dict(margin=1.625))                       # t_end = 0.1875 == t_in of voxel 2
    c['min_eq_max'] = ('posts', POST_T, POST_O, dict(min_range=1.0, max_range=1.0))
    c['min_above_max'] = ('posts', POST_T, POST_O, dict(min_range=1.5, max_range=1.0))
    c['min_above_target'] = ('posts', POST_T, POST_O, dict(min_range=2.0))
    c['zero_length'] = ('posts', POST_O.astype(np.float32), POST_O, dict(max_range=1.0))
    c['steps1'] = ('posts', POST_T, POST_O, dict(max_steps=1))
    c['steps5'] = ('posts', POST_T, POST_O, dict(max_steps=5, min_range=0.9))                  # the hit would be visit 7
    c['steps_exact'] = ('posts', POST_T, POST_O, dict(max_steps=3))                            # the hit IS visit 3: HIT, not TRUNCATED
    c['steps_exact7'] = ('posts', POST_T, POST_O, dict(max_steps=7, min_range=0.9))
    c['steps_end'] = ('posts', POST_T, POST_O, dict(max_steps=9, min_range=1.9))               # the walk ends by itself at its 9th visit: MISS
    # invalid coordinates, first, last and alone
    good, org, _ = _block_rays(6, 3)
    bad = np.array([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [32768, 0, 0], [0, -32768, 0]], np.float32)
    c['bad_first'] = ('rows343', np.concatenate([bad, good]), org[:1], dict(max_range=0.9))
    c['bad_last'] = ('rows343', np.concatenate([good, bad]), org[:1], dict(max_range=0.9))
    for j in range(5):
        c['bad_alone%d' % j] = ('rows343', bad[j:j + 1], org[:1], dict(max_range=0.9))
    bad_o = np.array([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [0, 0, 32768.0], [-32768.0, 0, 0]])
    c['bad_origins_first'] = ('rows343', np.concatenate([good[:5], good]), np.concatenate([bad_o, org[:1]]),
                              dict(origin_index=np.array([0, 1, 2, 3, 4] + [5] * 6, np.int32), max_range=0.9))
    c['bad_origins_last'] = ('rows343', np.concatenate([good, good[:5]]), np.concatenate([bad_o, org[:1]]),
                             dict(origin_index=np.array([5] * 6 + [0, 1, 2, 3, 4], np.int32), max_range=0.9))
    for j in range(5):
        c['bad_origin_alone%d' % j] = ('rows343', good[:1], bad_o[j:j + 1], dict(max_range=0.9))
    c['bad_index'] = ('rows343', good[:4], np.concatenate([org[:1], org[:1]]), dict(origin_index=np.array([-1, 0, 2, 1], np.int32), max_range=0.9))
    # the index bound: outwards through the last voxel of every axis at both ends; the decoys are never hit
    ends, starts, index, _ = _bound_rays()
    c['bound_first'] = ('bound', ends, starts, dict(origin_index=index, max_range=0.1))
    c['bound_last'] = ('bound', ends, starts, dict(origin_index=index, max_range=0.1, min_range=0.012))
    c['bound_through'] = ('bound', ends, starts, dict(origin_index=index, max_range=0.1, min_range=0.03))
    # accum_keep's ratio boundaries: one ray to the centre of every voxel of RATIO_SPEC
    rays = ah.centres([v for v, _, _ in RATIO_SPEC], 1.0)
    for k, (flt, _) in enumerate(RATIO_FILTERS):
        c['ratio_filter%d' % k] = ('ratio', rays, np.array([[0.5, 0.5, 0.5]]), dict(flt))
    # a filtered-out voxel in front of a kept one is transparent
    along = (np.array([[0.55, 0.05, 0.05]], np.float32), np.array([[-0.15, 0.05, 0.05]]))
    for tag, flt in (('none', dict()), ('fraction0', dict(max_moving_fraction=0.0)), ('count3', dict(min_count=3)), ('count4', dict(min_count=4)),
                     ('count6', dict(min_count=6))):
        c['transparent_' + tag] = ('filter',) + along + (flt,)
    # occlusion: a second wall behind the first
    far = ah.centres([(40, y, z) for y, z in WALL_YZ[::7]], 0.1)
    c['walls_near'] = ('walls', far, SENSOR, dict())
    c['walls_min_range'] = ('walls', far, SENSOR, dict(min_range=3.75))
    c['walls_min_count'] = ('walls', far, SENSOR, dict(min_count=2))
    c['ghost'] = ('ghost', _scan_of_the_ghost_scene(), SENSOR, dict(max_range=30.0))
    return c


CASES = _cases()
CASE_NAMES = sorted(CASES)


# ---- the host build and the restatement, each computed once per case ------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_raycast_host_driver', 'raycast_host')


def _run_host(exe, tmp_path, tag, records, targets, origins, voxel_size, spare=3, origin_index=None, pose=None, max_range=None, min_range=0.0, margin=0.0,
              min_count=1, max_moving_fraction=None, max_steps=4096):
    keys, acc, _ = records
    m, n = keys.shape[0], targets.shape[0]
    origins = np.asarray(origins, np.float64).reshape(-1, 3)
    head = [n, origins.shape[0], m, m + spare, max_steps, 0 if origin_index is None else 1, 0 if pose is None else 1, min_count,
            0 if max_moving_fraction is None else 1]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64),
                        np.array([voxel_size, min_range, -1.0 if max_range is None else max_range, margin,
                                  0.0 if max_moving_fraction is None else max_moving_fraction], np.float64),
                        np.ascontiguousarray(targets, np.float32), origins, b'' if origin_index is None else np.ascontiguousarray(origin_index, np.int32),
                        b'' if pose is None else np.ascontiguousarray(pose, np.float64), ah.map_bytes(keys, acc))
    out, off = ah.unpack(raw, 64, [(f, yref.DTYPES[f], (n, 3) if f in yref.WIDE else (n,)) for f in yref.FIELDS])
    assert off == len(raw)
    return dict(out, counters=np.frombuffer(raw, np.int64, 7).tolist(), kept=int(np.frombuffer(raw, np.int64, 1, 56)[0]))


_hosted, _restated = {}, {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, targets, origins, args = CASES[name]
        r = _scene(scene)
        _hosted[name] = _run_host(exe, tmp_path, name, r.records(), targets, origins, r.voxel_size, **args)
    return _hosted[name]


def _restate(name):
    """-> (columns and counters, the per-ray dicts) of a case."""
    if name not in _restated:
        scene, targets, origins, args = CASES[name]
        rays = []
        _restated[name] = (yref.raycast(_scene(scene), targets, origins, rays=rays, **args), rays)
    return _restated[name]


def _assert_same(got, want, what):
    assert list(got['counters']) == list(want['counters']), (what, got['counters'], want['counters'])
    for f in yref.FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert np.array_equal(ah.bits(got[f]), ah.bits(want[f])), (what, f, np.flatnonzero(ah.bits(got[f]).reshape(got[f].shape[0], -1) !=
                                                                                         ah.bits(want[f]).reshape(got[f].shape[0], -1))[:5])


def _assert_well_formed(res, voxel_size, what):
    """What holds for every result: the counters count the statuses, the defaults without a hit, and the bound on depth - range_in for every hit."""
    s, c = res['status'], list(res['counters'])
    assert c[:6] == [len(s)] + [int((s == k).sum()) for k in (DROPPED, SKIPPED, HIT, MISS, TRUNCATED)] and c[6] == int(res['visits'].sum()), what
    hit = s == HIT
    assert (res['row'][~hit] == -1).all() and np.isposinf(res['range_in'][~hit]).all() and np.isposinf(res['depth'][~hit]).all(), what
    assert (res['coords'][~hit] == 0).all() and (res['point'][~hit] == 0).all() and (res['length'][s == DROPPED] == 0).all(), what
    assert (res['visits'][(s == DROPPED) | (s == SKIPPED)] == 0).all() and (res['visits'][hit | (s == MISS) | (s == TRUNCATED)] >= 1).all(), what
    assert (res['row'][hit] >= 0).all() and (res['range_in'][hit] >= 0).all(), what
    assert (np.abs(res['depth'][hit] - res['range_in'][hit]) <= _bound_on_depth(voxel_size)).all(), what      # the bound of csrc/accum_raycast.h


# ---- CPU: host build == restatement -------------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    assert [_scene('rows%d' % m).num_voxels for m in (0, 1, 65, 343)] == [0, 1, 65, 343]
    walked, decoys = ah.walked_voxels()
    assert _scene('bound').num_voxels == len(set(walked + decoys)) and len(decoys) == 4
    assert 20000 < _scene('third').num_voxels < 22500 and 1100 < _scene('sparse').num_voxels < 1500
    assert np.rad2deg(np.arccos((np.trace(POSE[:3, :3]) - 1) / 2)) > 10.0                    # no pose near the identity


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want, got = _restate(name)[0], _host(host_exe, tmp_path, name)
    _assert_same(got, want, name)
    _assert_well_formed(got, _scene(CASES[name][0]).voxel_size, name)
    assert got['kept'] == len(qref.kept_voxels(_scene(CASES[name][0]), CASES[name][3].get('min_count', 1), CASES[name][3].get('max_moving_fraction')))


def test_sizes_and_validity():
    for n in RAY_COUNTS:
        empty = _restate('n%d_rows0' % n)[0]
        assert empty['counters'][0] == n and empty['counters'][3] == 0 and set(empty['status'].tolist()) <= {MISS}      # m = 0: every valid ray misses
        full = _restate('n%d_rows343' % n)[0]
        assert full['counters'][0] == n and (n < 63 or full['counters'][3] > n // 2)
    assert _restate('n257_rows343')[0]['counters'][1:3] == [0, 0]
    first, last = _restate('bad_first')[0], _restate('bad_last')[0]
    assert (first['status'][:5] == DROPPED).all() and (first['status'][5:] != DROPPED).all() and first['counters'][1] == 5
    for f in yref.FIELDS:
        assert np.array_equal(ah.bits(first[f][:5]), ah.bits(last[f][-5:])) and np.array_equal(ah.bits(first[f][5:]), ah.bits(last[f][:-5])), f
    first, last = _restate('bad_origins_first')[0], _restate('bad_origins_last')[0]
    assert (first['status'][:5] == DROPPED).all() and (first['status'][5:] != DROPPED).all() and (last['status'][-5:] == DROPPED).all()
    assert np.array_equal(first['status'][5:], last['status'][:6]) and (first['status'][5:] == HIT).sum() >= 1
    for j in range(5):
        assert _restate('bad_alone%d' % j)[0]['counters'] == [1, 1, 0, 0, 0, 0, 0] and _restate('bad_origin_alone%d' % j)[0]['counters'] == [1, 1, 0, 0, 0, 0, 0]
    assert _restate('bad_index')[0]['status'].tolist()[::2] == [DROPPED, DROPPED] and DROPPED not in _restate('bad_index')[0]['status'].tolist()[1::2]
    res, rays = _restate('random')
    assert res['counters'][1:3] == [0, 0] and res['counters'][3] > 300 and res['counters'][5] == 0
    assert all(any(v == 0.0 for v in rays[k]['geom'][1]) for k in range(22))      # the rays with a zero component walk too


def test_exact_ties_and_the_face_start():
    """Voxel size 0.25, (0,0,0) -> (1,1,1): all three t_a are equal at every step and the tie goes to x, then y, then z.  Only the last voxel of the
    written-down walk is kept: it is the hit, and visits is the length of the list."""
    walk = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    res, rays = _restate('ties')
    assert [c for c, _ in rays[0]['visited']] == walk and res['status'].tolist() == [HIT] and res['visits'].tolist() == [len(walk)]
    assert res['coords'].tolist() == [[3, 3, 3]] and res['range_in'][0] == 0.75 * math.sqrt(3.0) and res['depth'][0] == (0.875 * 3) / math.sqrt(3.0)
    # the origin on the face x = 0.5 of voxel 2, direction -x: t_x = -0.0 at the first step, the ray leaves voxel 2 at once
    res, rays = _restate('face')
    assert [c for c, _ in rays[0]['visited']] == [(2, 1, 1), (1, 1, 1), (0, 1, 1), (-1, 1, 1)] and res['coords'].tolist() == [[-1, 1, 1]]
    res, rays = _restate('face_next')
    assert res['status'].tolist() == [HIT] and res['visits'].tolist() == [2] and res['range_in'][0] == 0.0 and np.signbit(res['range_in'][0])


def test_exact_boundaries_of_the_extent():
    """The posts: d = (2, 0, 0), L = 2, voxel k entered at range 0.25 k - 0.125, every number exact."""
    want = {'inside': (HIT, 2, 1, 0.0), 'plain': (HIT, 2, 3, 0.375), 'min_range_on': (HIT, 2, 3, 0.375), 'min_range_above': (HIT, 4, 5, 0.875),
            'min_range_above_last': (MISS, 0, 9, INF), 'max_range_on': (MISS, 0, 2, INF), 'max_range_above': (HIT, 2, 3, 0.375),
            'max_range_past_target': (HIT, 2, 3, 0.375), 'margin_in_front': (MISS, 0, 2, INF),
            'max_range_zero': (SKIPPED, 0, 0, INF), 'margin_L': (SKIPPED, 0, 0, INF), 'margin_above_L': (SKIPPED, 0, 0, INF), 'min_eq_max': (SKIPPED, 0, 0, INF),
            'min_above_max': (SKIPPED, 0, 0, INF), 'min_above_target': (SKIPPED, 0, 0, INF), 'zero_length': (SKIPPED, 0, 0, INF),
            'steps1': (TRUNCATED, 0, 1, INF), 'steps5': (TRUNCATED, 0, 5, INF), 'steps_exact': (HIT, 2, 3, 0.375), 'steps_exact7': (HIT, 6, 7, 1.375),
            'steps_end': (MISS, 0, 9, INF)}
    for name, (status, x, visits, range_in) in want.items():
        res = _restate(name)[0]
        assert (int(res['status'][0]), int(res['coords'][0, 0]), int(res['visits'][0]), float(res['range_in'][0])) == (status, x, visits, range_in), name
        assert float(res['length'][0]) == (0.0 if name == 'zero_length' else 0.125 if name == 'max_range_past_target' else 1.5 if name == 'inside' else 2.0)
        if status == HIT:
            assert float(res['depth'][0]) == range_in + (0.125 if name != 'inside' else 0.0) and res['point'][0].tolist() == [0.25 * x + 0.125, 0.125, 0.125]


def test_index_bound_and_decoys():
    """Rays that leave the grid through the last voxel of an axis stop there: MISS, and no decoy is ever the hit."""
    walked, decoys = ah.walked_voxels()
    ends = _bound_rays()[3]
    first, last, through = (_restate(n)[0] for n in ('bound_first', 'bound_last', 'bound_through'))
    for res in (first, last, through):
        assert res['status'][6:].tolist() == [DROPPED, DROPPED]
        assert all(tuple(c) not in decoys for c in res['coords'][res['status'] == HIT].tolist())
    assert (first['status'][:6] == HIT).all() and (first['visits'][:6] == 1).all()
    assert (last['status'][:6] == HIT).all() and last['coords'][:6].tolist() == [list(e) for e in ends] and (last['visits'][:6] == 3).all()
    assert (through['status'][:6] == MISS).all() and (through['visits'][:6] == 3).all()          # the walk ends where the index would leave [-2^20, 2^20)


def test_filter_cases():
    for k, (_, n) in enumerate(RATIO_FILTERS):                                    # filter ratios exactly on a record's ratio
        res = _restate('ratio_filter%d' % k)[0]
        assert res['counters'][3:5] == [n, 7 - n], k
        assert all(res['coords'][j].tolist() == list(RATIO_SPEC[j][0]) for j in np.flatnonzero(res['status'] == HIT))
    want = {'none': (0, 3), 'fraction0': (1, 4), 'count3': (0, 3), 'count4': (3, 6), 'count6': (0, 8)}
    for tag, (x, visits) in want.items():                                         # a voxel the filter drops is transparent
        res = _restate('transparent_' + tag)[0]
        assert (int(res['coords'][0, 0]), int(res['visits'][0]), int(res['status'][0])) == (x, visits, MISS if tag == 'count6' else HIT), tag
    assert _restate('transparent_fraction0')[0]['row'].tolist() == [0] and _restate('transparent_count4')[0]['row'].tolist() == [0]
    assert _restate('transparent_none')[0]['row'].tolist() == [0] and _restate('rows343_filtered')[0]['counters'][3] > 50


# ---- CPU: the restatement against the geometry of the ray --------------------------------------------------------------------------------------------------
def _chord(o, d, lo, hi, t_end):
    """The segment o + t d, t in [0, t_end], against the boxes [lo, hi] ([V,3] each) -> (t0, t1) [V]: inside for t0 <= t <= t1, none when t1 < t0."""
    t0, t1 = np.zeros(lo.shape[0]), np.full(lo.shape[0], t_end)
    with np.errstate(all='ignore'):
        for a in range(3):
            if d[a] == 0.0:
                out = (o[a] < lo[:, a]) | (o[a] > hi[:, a])
                t0, t1 = np.where(out, 1.0, t0), np.where(out, 0.0, t1)
            else:
                ta, tb = (lo[:, a] - o[a]) / d[a], (hi[:, a] - o[a]) / d[a]
                t0, t1 = np.maximum(t0, np.minimum(ta, tb)), np.minimum(t1, np.maximum(ta, tb))
    return t0, t1


def test_the_hit_is_the_first_kept_voxel_the_ray_crosses():
    """300 random rays through 2 % of a 40^3 block at 0.25 m, max_range 4 m.  The hit voxel's box grown by 1e-9 m is crossed by the ray; no kept voxel
    whose box shrunk by 1e-9 m holds a chord longer than 1e-9 m is entered earlier; a ray with such a must-hit voxel never misses.  A ray whose
    decision falls inside the band is excluded: at most 1 % of the rays."""
    r = _scene('sparse')
    vs = r.voxel_size
    rs = np.random.RandomState(17)
    origins = rs.uniform(-1.0, 1.0, (3, 3))
    targets = (origins[0] + rs.normal(0, 1, (300, 3))).astype(np.float32)
    rays = []
    res = yref.raycast(r, targets, origins, origin_index=rs.randint(0, 3, 300), max_range=4.0, rays=rays)
    idx = np.array([c for c, _ in qref.kept_voxels(r)], np.float64)
    lo, hi = idx * vs, (idx + 1) * vs
    row_of = {tuple(int(v) for v in c): j for j, c in enumerate(idx.tolist())}
    band = 0
    for k, ray in enumerate(rays):
        o, d, L, t_start, t_end = ray['geom']
        o, d = np.array(o), np.array(d)
        assert ray['status'] in (HIT, MISS) and t_start == 0.0 and abs(t_end * L - 4.0) < 1e-12
        g0, g1 = _chord(o, d, lo - EPS, hi + EPS, t_end)
        s0, s1 = _chord(o, d, lo + EPS, hi - EPS, t_end)
        must = (s1 - s0) * L > EPS
        if ray['status'] == MISS:
            assert not must.any(), (k, idx[must][:3])                             # a ray with a must-hit voxel never misses
            band += int((g1 >= g0).any())                                         # it grazed a kept voxel within the band
            continue
        j = row_of[ray['coords']]
        assert g1[j] >= g0[j], k                                                  # the hit voxel (grown) is crossed
        b0, _ = _chord(o, d, lo[j:j + 1], hi[j:j + 1], t_end)
        assert abs(ray['range_in'] - b0[0] * L) <= EPS, k                         # ... and range_in is where the ray enters it
        earlier = must & (s0 * L < ray['range_in'] - EPS)
        earlier[j] = False
        assert not earlier.any(), (k, idx[earlier][:3])                           # no must-hit voxel is entered earlier
        band += int(not must[j])
    print('%d hits, %d misses, %d rays in the band' % (res['counters'][3], res['counters'][4], band))
    assert res['counters'][3] > 90 and res['counters'][4] > 90 and band <= 3


def test_depth_bound_on_random_centroids():
    """|depth - range_in| <= sqrt(3) voxel_size + 2^-17 + 1e-9 on a map whose centroids lie anywhere in their voxels (the scenes above keep them in the
    middle): the 'third' block filled with random points."""
    rs = np.random.RandomState(23)
    pts = rs.uniform(-1.0, 1.0, (6000, 3)).astype(np.float32)
    r = ah.points_map(0.1, [(pts, None, 0)])
    targets, origins, index = ah.random_rays()
    res = yref.raycast(r, targets, origins, origin_index=index, max_range=3.0)
    _assert_well_formed(res, 0.1, 'random centroids')
    hit = res['status'] == HIT
    assert hit.sum() > 300 and np.abs(res['depth'][hit] - res['range_in'][hit]).max() > 0.05
    e = r.extract()
    assert np.array_equal(e['points'][res['row'][hit]], res['point'][hit]) and np.array_equal(e['coords'][res['row'][hit]], res['coords'][hit])


# ---- CPU: what the ray cast is for ------------------------------------------------------------------------------------------------------------------------------
def test_occlusion_on_the_restatement():
    """Two walls: every ray that crosses both hits the nearer one; with min_range between the walls, or with the nearer wall (built at count 1) filtered
    out by min_count = 2, it hits the farther one."""
    near, by_range, by_count = (_restate(n)[0] for n in ('walls_near', 'walls_min_range', 'walls_min_count'))
    assert (near['status'] == HIT).all() and (near['coords'][:, 0] == 30).all() and len(near['status']) > 100
    for res in (by_range, by_count):
        assert (res['status'] == HIT).all() and (res['coords'][:, 0] == 40).all()
        assert (res['depth'] - near['depth'] > 0.9).all()
    assert np.array_equal(by_count['coords'], by_range['coords']) and by_count['row'].max() < len(WALL_YZ)       # rows of the filtered extract


def _ghost_classes():
    """The scan of the ghost scene by geometry alone: (cluster, behind, clear) masks.  behind: wall points whose ray crosses a GHOST voxel grown by
    1e-9 m; clear: wall points whose ray stays out of every GHOST voxel grown by 1e-9 m.  No wall point is neither."""
    scan = _scan_of_the_ghost_scene()
    g = np.array(GHOST, np.float64)
    o = SENSOR[0]
    behind = np.zeros(len(scan), bool)
    for k in range(len(WALL_YZ)):
        t0, t1 = _chord(o, scan[k].astype(np.float64) - o, g * 0.1 - EPS, (g + 1) * 0.1 + EPS, 1.0)
        s0, s1 = _chord(o, scan[k].astype(np.float64) - o, g * 0.1 + EPS, (g + 1) * 0.1 - EPS, 1.0)
        behind[k] = (t1 >= t0).any()
        assert behind[k] == (s1 > s0).any(), k                                    # no ray grazes the ghost within the band
    cluster = np.arange(len(scan)) >= len(WALL_YZ)
    return scan, cluster, behind, ~cluster & ~behind


def _assert_ghost_classes(depth, length, behind_is_empty=False):
    scan, cluster, behind, clear = _ghost_classes()
    tau = 2 * 0.1
    assert tau > math.sqrt(3.0) * 0.1 + 2.0 ** -17
    assert cluster.sum() == 27 and behind.sum() > 30 and clear.sum() > 600
    assert (depth[cluster] - length[cluster] > tau).all()                         # new object: the map's surface lies well behind the point
    if behind_is_empty:
        assert not (length - depth > tau).any()
        assert (np.abs(depth[behind | clear] - length[behind | clear]) <= tau).all()
    else:
        assert (length[behind] - depth[behind] > tau).all()                       # seen through: this beam went through something the map holds
        assert (np.abs(depth[clear] - length[clear]) <= tau).all()                # consistent
    return scan


def test_new_objects_and_ghosts_on_the_restatement():
    res = _restate('ghost')[0]
    _assert_ghost_classes(res['depth'], res['length'])
    assert res['counters'][1:3] == [0, 0] and res['counters'][5] == 0


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_raycast_workspace_bytes', 'pcacc_accum_raycast'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C10. ' in header and len(native._PROTOTYPES['pcacc_accum_raycast']) == 30
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_raycast.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_normals.h"', '#include "accum_pierce.h"']
    for helper in ('accp_end_point(', 'accp_origin_index', 'accp_in_range', 'accp_step(', 'accum_key(', 'accum_lower_bound(', 'accum_field(', 'accn_index(',
                   'accn_centroid('):
        assert helper in text, helper
    assert 'PCACC_NO_CONTRACT' in text
    pierce = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_pierce.h')).read()
    assert pierce.count('accp_step(') >= 2 and pierce.count('t < t_best') == 1     # one copy of the step: C7 walks with it too
    kernel = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_raycast.hip')).read()
    assert kernel.count('__global__') == 1 and 'accy_ray_kernel' in kernel and 'accum_wave_count(' in kernel and 'asm(' not in kernel and 'asm volatile' not in kernel
    assert '__shfl_xor' in open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_launch.h')).read()      # the wave reduction behind accum_wave_count
    assert (native.RAYCAST_MISS, native.RAYCAST_HIT, native.RAYCAST_TRUNCATED, native.RAYCAST_SKIPPED, native.RAYCAST_DROPPED, native.RAYCAST_COUNTERS) == \
        (0, 1, 2, 3, 4, 7)
    for k, name in enumerate(('RAYS', 'DROPPED', 'SKIPPED', 'HIT', 'MISSED', 'TRUNCATED', 'VISITS')):
        assert getattr(native, 'RAYCAST_N_' + name) == k and ('#define PCACC_RAYCAST_N_%s %d\n' % (name, k)) in header
    assert 'accum_raycast.hip' in open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'Makefile')).read()
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.raycast(torch.zeros(4, 3), np.zeros(3))
    with pytest.raises(native.NativeError):
        cpu.render_range_image(None, 2, 4, 0.1, -0.1, 5.0)
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).raycast(np.zeros((4, 3), np.float32), np.zeros(3))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
_clouds = {}


def _cloud(scene):
    """A device map per scene, shared: raycast does not modify it (a test below says so)."""
    if scene not in _clouds:
        _clouds[scene] = ah.device_cloud(_scene(scene))
    return _clouds[scene]


def _cast(m, targets, origins, args):
    a = dict(args)
    if a.get('origin_index') is not None:
        a['origin_index'] = torch.from_numpy(np.ascontiguousarray(a['origin_index'])).to(DEV)
    return m.raycast(torch.from_numpy(np.ascontiguousarray(targets, np.float32)).to(DEV), origins, **a)


def _assert_device_equals(res, want, what):
    """torch.equal on every column and on the counters; floats also as their bits (+inf, -0.0 and every last bit)."""
    assert sorted(res) == sorted(yref.FIELDS + ('counters',))
    assert res['counters'].dtype == torch.int64 and res['counters'].tolist() == list(want['counters']), (what, res['counters'].tolist(), want['counters'])
    for f in yref.FIELDS:
        w = torch.from_numpy(want[f]).to(DEV)
        assert res[f].is_cuda and res[f].dtype == w.dtype and res[f].shape == w.shape, (what, f)
        if w.dtype.is_floating_point:
            assert torch.equal(res[f].view(torch.int64 if w.dtype == torch.float64 else torch.int32), torch.from_numpy(ah.bits(want[f])).to(DEV)), (what, f)
        assert torch.equal(res[f], w), (what, f)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    scene, targets, origins, args = CASES[name]
    host = _host(host_exe, tmp_path, name)
    m = _cloud(scene)
    snap = ah.snapshot(m, whole_sidecar=True)
    res = _cast(m, targets, origins, args)
    _assert_device_equals(res, host, name)
    again = _cast(m, targets, origins, args)                                      # a second run gives the same bits
    assert all(torch.equal(res[f], again[f]) for f in res)
    ah.assert_unchanged(m, snap, name)                                              # read-only: keys, records, stamps, sidecar, state words, num_voxels


def _short_rays(n=70001):
    """n rays of 0.3 - 1.5 m that end on the wavy sheet (jittered), each from its own origin, mostly from above."""
    rs = np.random.RandomState(77)
    targets = ah.wavy()[rs.randint(0, 270400, n)] + rs.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)
    direction = rs.normal(0, 1, (n, 3))
    direction[:, 2] = np.abs(direction[:, 2]) + 0.3
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    origins = targets.astype(np.float64) + direction * rs.uniform(0.3, 1.5, (n, 1))
    return targets, origins, np.arange(n, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('args', [dict(), dict(max_range=2.0, min_range=0.1, min_count=4, pose=ah.rot_xyz(0.002, -0.001, 0.003, (0.01, 0.02, -0.01)))],
                         ids=['to_target', 'range_filtered_pose'])
def test_kernel_on_76661_voxels_and_70001_rays_gpu(host_exe, tmp_path, args):
    r = _scene('wavy')
    targets, origins, index = _short_rays()
    n = targets.shape[0]
    assert r.num_voxels == 76661 and n == 70001 and n % 64 != 0 and n % 256 != 0
    host = _run_host(host_exe, tmp_path, 'wavy', r.records(), targets, origins, r.voxel_size, origin_index=index, **args)
    m = _cloud('wavy')
    snap = ah.snapshot(m, whole_sidecar=True)
    res = _cast(m, targets, origins, dict(args, origin_index=index))
    _assert_device_equals(res, host, 'wavy')
    _assert_well_formed(host, r.voxel_size, 'wavy')
    assert host['counters'][3] > 20000 and host['counters'][4] > 100 and host['counters'][1] == host['counters'][2] == 0
    assert all(torch.equal(res[f], v) for f, v in _cast(m, targets, origins, dict(args, origin_index=index)).items())
    ah.assert_unchanged(m, snap, 'wavy')


@pytest.mark.gpu
def test_identities_with_extract_gpu():
    from pcaccumulation_amd import native
    r = ah.points_map(0.1, [(np.random.RandomState(23).uniform(-1.0, 1.0, (6000, 3)).astype(np.float32), None, 0),
                          (np.random.RandomState(24).uniform(-1.0, 1.0, (3000, 3)).astype(np.float32), np.arange(3000) % 5 == 0, 1)])
    m = ah.device_cloud(r)
    targets, origins, index = ah.random_rays()
    for f in (dict(), dict(min_count=2, max_moving_fraction=0.0)):
        e = m.extract(**f)
        res = _cast(m, targets, origins, dict(f, origin_index=index, max_range=3.0))
        s = res['status']
        hit = s == HIT
        assert int(hit.sum()) > 100
        assert torch.equal(res['point'][hit], e['points'][res['row'][hit].long()]) and torch.equal(res['coords'][hit], e['coords'][res['row'][hit].long()])
        want = [400] + [int((s == k).sum()) for k in (DROPPED, SKIPPED, HIT, MISS, TRUNCATED)] + [int(res['visits'].sum())]
        assert res['counters'].tolist() == want
        _assert_device_equals(res, yref.raycast(r, targets, origins, origin_index=index, max_range=3.0, **f), 'identities')
        # from one origin at every centroid extract returns, to the target: the ray reaches the centroid's voxel, so every ray is a HIT in front of it
        own = m.raycast(e['points'], np.array([0.013, -0.021, 0.017]), max_range=None, margin=0.0, **f)
        assert bool((own['status'] == HIT).all()) and bool((own['range_in'] <= own['length']).all())
        assert own['counters'].tolist()[:6] == [e['points'].shape[0], 0, 0, e['points'].shape[0], 0, 0]
    assert native.RAYCAST_FIELDS[0][0] == 'status' and [name for name, _, _ in native.RAYCAST_FIELDS] == list(yref.FIELDS)


@pytest.mark.gpu
def test_tie_to_see_through_gpu():
    """On a fresh sidecar, after see_through of the same rays with the same margin and no stamp, every voxel raycast(max_range=None, min_count=1) hits
    has pierced >= 1: the two walk the same voxels.  When see_through's hit counter stays 0, no ray hits."""
    from pcaccumulation_amd import native
    targets, origins, index = ah.random_rays()
    pts, idx = torch.from_numpy(targets).to(DEV), torch.from_numpy(index).to(DEV)
    m = ah.device_cloud(_scene('third'))
    counters = m.see_through(pts, origins, idx, margin=0.2)
    res = m.raycast(pts, origins, idx, max_range=None, margin=0.2, min_count=1)
    hit = res['status'] == HIT
    assert int(hit.sum()) > 300 and int(counters[native.PIERCE_HITS]) >= int(hit.sum())
    assert bool((m.pierced()[res['row'][hit].long()] >= 1).all())
    assert int(counters[native.PIERCE_WALKED]) == 400 - int((res['status'] == SKIPPED).sum()) - int((res['status'] == DROPPED).sum())
    away = ah.device_cloud(ah.records(0.1, {(25, 25, 25): (1, 0), (-25, 25, 25): (1, 0)}))
    counters = away.see_through(pts, origins, idx, margin=0.2)
    res = away.raycast(pts, origins, idx, max_range=None, margin=0.2, min_count=1)
    assert int(counters[native.PIERCE_HITS]) == 0 and int(counters[native.PIERCE_WALKED]) > 380 and not bool((res['status'] == HIT).any())


@pytest.mark.gpu
def test_new_objects_and_ghosts_gpu():
    """The restatement's classes on the device, and after see_through of the scan and prune(min_pierced=1) no beam goes through anything the map holds."""
    r = _scene('ghost')
    m = ah.device_cloud(r)
    scan = _assert_ghost_classes(*(_restate('ghost')[0][f] for f in ('depth', 'length')))
    res = _cast(m, scan, SENSOR, dict(max_range=30.0))
    _assert_device_equals(res, _restate('ghost')[0], 'ghost')
    _assert_ghost_classes(res['depth'].cpu().numpy(), res['length'].cpu().numpy())
    m.see_through(torch.from_numpy(scan).to(DEV), SENSOR)
    pruned = m.prune(min_pierced=1)
    assert 0 < pruned['pierced'] <= 27 and pruned['kept'] >= len(WALL_YZ)
    after = _cast(m, scan, SENSOR, dict(max_range=30.0))
    _assert_ghost_classes(after['depth'].cpu().numpy(), after['length'].cpu().numpy(), behind_is_empty=True)
    pierced, reference = {}, ref.ReferenceMap(0.1)
    reference.rec = {k: list(v) for k, v in r.rec.items()}
    pref.pierce(pref.voxels_of(reference), scan, SENSOR, voxel_size=0.1, pierced=pierced)
    assert rref.prune(reference, pierced, min_pierced=1)[4] == pruned['pierced']
    _assert_device_equals(after, yref.raycast(reference, scan, SENSOR, max_range=30.0), 'ghost after prune')


@pytest.mark.gpu
def test_occlusion_gpu():
    m = _cloud('walls')
    for name in ('walls_near', 'walls_min_range', 'walls_min_count'):
        _assert_device_equals(_cast(m, *CASES[name][1:]), _restate(name)[0], name)


@pytest.mark.gpu
def test_render_range_image_gpu():
    m = _cloud('walls')
    pose = np.eye(4)
    pose[:3, 3] = SENSOR[0]
    img = m.render_range_image(pose, 8, 64, 0.2, -0.2, 30.0)
    assert sorted(img) == sorted(yref.FIELDS + ('counters', 'directions'))
    for f in yref.FIELDS:
        assert tuple(img[f].shape) == ((8, 64, 3) if f in yref.WIDE else (8, 64)), f
    d = img['directions']
    assert tuple(d.shape) == (8, 64, 3) and d.dtype == torch.float32 and tuple(img['counters'].shape) == (7,)
    el = 0.2 - (np.arange(8) + 0.5) * 0.4 / 8
    az = np.pi - (np.arange(64) + 0.5) * 2 * np.pi / 64
    want = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.sin(el)[:, None] * np.ones(64)[None, :]], -1)
    assert np.array_equal(d.cpu().numpy(), want.astype(np.float32))
    same = m.raycast(d.reshape(-1, 3), np.zeros(3), pose=pose, max_range=30.0)     # equals raycast on its own returned directions
    for f in yref.FIELDS:
        assert torch.equal(img[f].reshape(same[f].shape), same[f]), f
    assert torch.equal(img['counters'], same['counters'])
    _assert_device_equals(same, yref.raycast(_scene('walls'), d.reshape(-1, 3).cpu().numpy(), np.zeros((1, 3)), pose=pose, max_range=30.0), 'image')
    for r, c in ((3, 31), (4, 32)):                                               # the pixels around +x: the wall at x = 3.0 .. 3.1, the sensor at x = 0.03
        assert float(d[r, c, 0]) > 0.998 and int(img['status'][r, c]) == HIT and abs(float(img['depth'][r, c]) - 3.02) <= 0.1
        assert img['coords'][r, c].tolist()[0] == 30
    assert int(img['status'][3, 0]) == MISS and math.isinf(float(img['depth'][3, 0]))        # looking along -x: nothing
    filtered = m.render_range_image(pose, 8, 64, 0.2, -0.2, 30.0, min_count=2)
    assert abs(float(filtered['depth'][3, 31]) - 4.02) <= 0.1
    for bad in (dict(height=0), dict(width=0), dict(fov_up=NAN), dict(max_range=None)):
        with pytest.raises(ValueError):
            m.render_range_image(**dict(dict(pose=pose, height=8, width=64, fov_up=0.2, fov_down=-0.2, max_range=30.0), **bad))


def _both_add(m, r, pts, stamp, pose=None):
    m.add(torch.from_numpy(pts).to(DEV), pose, stamp=stamp)
    r.add(pts, pose, stamp=stamp)


def _assert_raycast_equals_restatement(m, r, targets, origins, what, **args):
    got = _cast(m, targets, origins, args)
    _assert_device_equals(got, yref.raycast(r, targets, origins, **args), what)
    e = m.extract(args.get('min_count', 1), args.get('max_moving_fraction'))      # `row` refers to the rows of the extract of that moment
    hit = got['status'] == HIT
    assert torch.equal(e['points'][got['row'][hit].long()], got['point'][hit]) and torch.equal(e['coords'][got['row'][hit].long()], got['coords'][hit]), what
    return got


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, pierced = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), {}
    origin = np.array([[0.05, 0.05, 0.05]])
    slab = ah.centres([(x, y, z) for x in (5, 6, 7) for y in range(-2, 3) for z in (-1, 0, 1)], 0.1)
    behind = ah.centres([(20, y, z) for y in (-4, -2, 0, 3, 5) for z in (-2, 0, 2)], 0.1)
    rays = np.concatenate([behind, slab[::3] + np.float32(0.03), ah.centres([(-9, 0, 0), (6, 9, 9)], 0.1), [[NAN, 0, 0]]]).astype(np.float32)
    _both_add(m, r, np.concatenate([slab, slab[::2]]), 0)
    a = _assert_raycast_equals_restatement(m, r, rays, origin, 'after add', max_range=3.0, min_count=2)
    every = _assert_raycast_equals_restatement(m, r, rays, origin, 'after add, all', max_range=3.0)
    assert 0 < int(a['counters'][3]) <= int(every['counters'][3])
    m.see_through(torch.from_numpy(behind).to(DEV), origin, stamp=1)
    pref.pierce(pref.voxels_of(r), behind, origin, voxel_size=0.1, stamp=1, pierced=pierced)
    b = _assert_raycast_equals_restatement(m, r, rays, origin, 'after see_through', max_range=3.0, min_count=2)
    assert all(torch.equal(a[f], b[f]) for f in a)                                # the sidecar is nothing to a ray cast
    assert m.prune(min_pierced=1)['pierced'] == rref.prune(r, pierced, min_pierced=1)[4] > 0
    c = _assert_raycast_equals_restatement(m, r, rays, origin, 'after prune', max_range=3.0)
    assert int(c['counters'][3]) < int(every['counters'][3])                       # the rays that went through the slab now find nothing
    _both_add(m, r, ah.centres([(-9, 0, 0), (6, 0, 0), (6, 0, 0), (6, 9, 9), (20, 0, 0)], 0.1), 2)
    d = _assert_raycast_equals_restatement(m, r, rays, origin, 'add after prune', max_range=3.0)
    assert int(d['counters'][3]) > int(c['counters'][3])
    path = os.path.join(str(tmp_path), 'map.npz')
    m.save(path)
    loaded = AccumulatedCloud.load(path, DEV)
    e = _assert_raycast_equals_restatement(loaded, r, rays, origin, 'after load', max_range=3.0)
    assert all(torch.equal(d[f], e[f]) for f in d)


@pytest.mark.gpu
def test_raycast_results_on_the_model_forward_gpu(golden):
    """raycast_results on the model_tiny_test forward: the counters sum to n and the result equals a direct raycast with hand-built origins.  Nothing more
    is claimed."""
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
    pose, offset = ah.rot_xyz(0, 0, 0.01, (0.02, -0.01, 0.0)), (0.1, -0.2, 1.8)
    res = m.raycast_results(out, inp, pose=pose, sensor_offset=offset, max_range=30.0)
    ego = out['ego_motion_est'][0].detach().double()
    origins = torch.stack([((ego[t, :3, 0] * offset[0] + ego[t, :3, 1] * offset[1]) + ego[t, :3, 2] * offset[2]) + ego[t, :3, 3] for t in range(ego.shape[0])])
    same = m.raycast(out['rec_est'], origins, inp['time_indice'][:, 1], pose, max_range=30.0)
    assert all(torch.equal(res[k], same[k]) for k in res)
    n = out['rec_est'].shape[0]
    assert int(res['counters'][0]) == n == int(res['counters'][1:6].sum())
    with pytest.raises(ValueError):
        m.raycast_results(dict(out, _n_batches=2), inp)


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    m = ah.device_cloud(_scene('rows65'))
    snap = ah.snapshot(m, whole_sidecar=True)
    n = 10
    targets, origins, index = _block_rays(n, 1)
    pts, org, idx = torch.from_numpy(targets).to(DEV), torch.from_numpy(origins).to(DEV), torch.from_numpy(index).to(DEV)
    out = {name: torch.full((n,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in native.RAYCAST_FIELDS}
    counters = torch.full((7,), 7, dtype=torch.int64, device=DEV)
    good = dict(targets=pts, origins=org, origin_index=idx, pose=None, voxel_size=0.1, min_range=0.0, max_range=1.0, margin=0.0, max_steps=4096, tables=m._cur,
                m=65, min_count=1, max_moving_fraction=None, out=out, counters=counters)
    for bad in (dict(m=-1), dict(m=m.capacity + 1), dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=INF), dict(voxel_size=NAN),
                dict(min_range=-0.1), dict(min_range=INF), dict(min_range=NAN), dict(margin=-0.1), dict(margin=INF), dict(margin=NAN), dict(max_range=NAN),
                dict(max_steps=0), dict(max_steps=(1 << 16) + 1), dict(origins=org[:0])):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_raycast(**dict(good, **bad))
    lib = native.lib()
    ptr = [native._dev(out[name]) for name, _, _ in native.RAYCAST_FIELDS]
    keys, acc, _ = (native._dev(t) for t in m._cur)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def call(n_rays=n, targets=native._dev(pts), origins=native._dev(org), ptr=ptr, keys=keys, acc=acc, cnt=native._dev(counters), ws=native._dev(ws),
             ws_bytes=ws.numel(), n_origins=3):
        return lib.pcacc_accum_raycast(targets, n_rays, origins, n_origins, native._dev(idx), None, 0.1, 0.0, 1.0, 0.0, 4096, keys, acc, m.capacity, 65, 1, 0, 0.0,
                                       *ptr, cnt, ws, ws_bytes, native._stream())
    assert call(n_rays=-1) == call(n_rays=(1 << 30) + 1) == call(targets=None) == call(origins=None) == call(keys=None) == call(acc=None) == -1
    assert call(cnt=None) == call(ws=None) == call(ws_bytes=16) == call(n_origins=0) == -1
    for k in range(len(ptr)):
        assert call(ptr=ptr[:k] + [None] + ptr[k + 1:]) == -1, k                  # a NULL output of non-zero size
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in list(out.values()) + [counters])     # nothing was launched: outputs and counters keep their poison
    ah.assert_unchanged(m, snap, 'bad arguments')
    for bad in (dict(min_range=-0.1), dict(min_range=INF), dict(margin=-1.0), dict(margin=NAN), dict(max_range=-1.0), dict(max_range=NAN), dict(max_steps=0),
                dict(max_steps=(1 << 16) + 1), dict(max_range=1.0, margin=0.1), dict(pose=np.eye(3)), dict(origin_index=idx[:5])):
        with pytest.raises(ValueError):
            m.raycast(pts, origins, **bad)
    for bad_targets, bad_origins in ((pts[:, :2], origins), (pts, np.zeros((0, 3))), (pts, np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            m.raycast(bad_targets, bad_origins)
    with pytest.raises(native.NativeError):
        m.raycast(pts.cpu(), origins)
    with pytest.raises(native.NativeError):
        m.raycast(pts, origins, idx.cpu())
    zero = native.accum_raycast(**dict(good, targets=pts[:0], origin_index=idx[:0], out={k: t[:0] for k, t in out.items()}))   # n = 0: the zero counters only
    assert zero['counters'].tolist() == [0] * 7 and all(bool((t == 7).all()) for t in out.values())
    assert call() == 0 and counters.tolist()[0] == n and not bool((out['status'] == 7).any())
    ah.assert_unchanged(m, snap, 'after all')
