"""Looking a scan's points up in the accumulated scene cloud (include/pcacc.h C9): AccumulatedCloud.query / query_results.

Every result is an integer, a copied record or a float64 computed by + - * / and sqrt in one order, so every claim is an equality of bits:
  CPU   the g++ build of csrc/accum_query.h (tests/accum_query_host_driver.cpp, every table index asserted, poison behind the rows in use and in every
        output, every output row written once) against the plain-Python restatement on coordinate dicts (tests/accumulate_query_reference.py), and the
        restatement against a brute-force nearest neighbour over ALL kept centroids for max_distance <= 0.9 voxel_size;
  GPU   the kernel against the g++ build on the same scenes, then identities that tie query to extract / pierced / register, a life cycle against the
        restatement, the ghost scene of section 9f and the novelty of drifting windows.
The one tolerance (1e-9 relative) is the rmse of register, whose sum runs in another order."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_pierce_reference as pref
import accumulate_prune_reference as rref
import accumulate_query_reference as qref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

I, O, K, M, N = qref.INVALID, qref.OCCUPIED, qref.KEPT, qref.MATCHED, qref.NORMAL


# ---- scenes: a ReferenceMap and a {coord: rays} dict (None: no sidecar), built once and never modified --------------------------------------------
# (voxel, points, moving): 1 of 4 sits exactly on 0.25; 1 of 3 and 2 of 4 above; 0 of 2 and 0 of 1 below; 4 of 4
RATIO_SPEC = [((2, 0, 0), 4, 1), ((-1, 3, 0), 3, 1), ((0, 0, 5), 4, 2), ((0, -2, 1), 2, 0), ((-7, 0, 0), 1, 0), ((2, 0, -1), 4, 4), ((0, 0, -5), 8, 2)]
RATIO_FILTERS = ((dict(min_count=1), 7), (dict(min_count=4), 4), (dict(min_count=5), 1), (dict(min_count=9), 0), (dict(max_moving_fraction=0.25), 4),
                 (dict(max_moving_fraction=float(np.nextafter(0.25, 0))), 2), (dict(max_moving_fraction=0.0), 2),
                 (dict(min_count=3, max_moving_fraction=1.0 / 3.0), 3), (dict(min_count=4, max_moving_fraction=0.25), 2),
                 (dict(max_moving_fraction=1.0), 7))


FILTER = dict(min_count=2, max_moving_fraction=0.0)


POSE = ah.rot_xyz(np.deg2rad(0.6), np.deg2rad(-0.5), np.deg2rad(0.7), (0.02, -0.015, 0.017))      # about 1 degree and 0.3 voxel of 0.1 m


def _corner_adds():
    pts = ah.corner(11, 3000).astype(np.float32)
    mv = (pts[:, 0] > ah.CORNER[0] + 1.6) & (np.random.RandomState(4).uniform(0, 1, pts.shape[0]) < 0.5)
    return [(pts[:5000], mv[:5000], 3), (pts[5000:], mv[5000:], 1)]


def _corner_scan(n=300):
    inv = np.linalg.inv(POSE)
    return (ah.corner(12, n) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


_scenes = {}


def _build_scene(name):
    if name == 'rows65_no_sidecar':
        return ah.records(0.1, ah.random_rows(65, 7)[0]), None
    if name == 'rows343_no_sidecar':
        return ah.records(0.1, ah.random_rows(343, 8)[0]), None
    if name.startswith('rows'):
        rows, pierced = ah.random_rows(int(name[4:]), 100 + int(name[4:]))
        return ah.records(0.1, rows), pierced
    if name == 'ratio':
        return ah.records(1.0, {v: (k, j, 0, 0) for v, k, j in RATIO_SPEC}), None
    if name == 'bound':
        vox, decoys = ah.bound_voxels()
        return ah.points_map(0.01, [(ah.centres(vox + decoys, 0.01), None, 0)]), None
    if name == 'tie':                                                              # 0.25 is exact: every centroid exactly at its voxel centre
        return ah.records(0.25, {(x, y, z): (1, 0, 0, 0) for x in (0, 1) for y in (0, 1) for z in (0, 1)}), None
    if name == 'filter':                                                           # (0,0,0) fails max_moving_fraction=0, (1,0,0) and (3,0,0) pass, (2,0,0) is empty
        return ah.records(0.1, {(0, 0, 0): (3, 1, 0, 2), (1, 0, 0): (2, 0, 1, 1), (3, 0, 0): (5, 0, 0, 4), (20, 20, 20): (1, 0, 0, 0)}), {(0, 0, 0): 3}
    if name == 'plane':
        return ah.points_map(0.1, [(ah.noisy_plane(), None, 0)]), None
    if name == 'corner':
        return ah.points_map(0.1, _corner_adds()), None
    if name == 'uniform':
        return ah.points_map(0.1, [(np.random.RandomState(5).uniform(-0.6, 0.6, (2500, 3)).astype(np.float32), None, 0)]), None
    assert name == 'wavy'
    return ah.points_map(0.1, [(ah.wavy(), None, 0)]), None


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene, the points and the arguments of one query -------------------------------------------------------------------------------------------
POINT_COUNTS = (0, 1, 63, 64, 65, 257)
INVALID_POINTS = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [32768.0, 0, 0], [0, -32768.0, 0], [10486.0, 0, 0], [0, 0, -10486.0]]   # the last two: index outside +-2^20 at 0.01 m
TIE_POINT = np.array([[0.25, 0.125, 0.125]], np.float32)


def _block_points(n, seed):
    """n points over the 7^3 block and a voxel beyond it on every side."""
    return np.random.RandomState(seed).uniform(-0.42, 0.52, (n, 3)).astype(np.float32)


def _bound_points():
    vox, _ = ah.bound_voxels()
    last = [v for v in vox if any(c in (-EDGE, EDGE - 1) for c in v)]                # the last voxel of each axis at both ends
    rs = np.random.RandomState(3)
    return np.concatenate([ah.centres(last, 0.01), ah.centres(last, 0.01) + rs.uniform(-0.002, 0.002, (len(last), 3)).astype(np.float32)]), last


def _cases():
    cases = {}
    for n in POINT_COUNTS:
        for scene in ('rows0', 'rows1', 'rows65', 'rows343', 'rows65_no_sidecar', 'rows343_no_sidecar'):
            cases['n%d_%s' % (n, scene)] = (scene, _block_points(n, n + 1), dict(max_distance=0.08))
    cases['n257_rows343_filtered'] = ('rows343', _block_points(257, 9), dict(min_count=2, max_moving_fraction=0.5))
    valid = _bound_points()[0][:20]
    bad = np.array(INVALID_POINTS, np.float32)
    cases['invalid_first'] = ('bound', np.concatenate([bad, valid]), dict())
    cases['invalid_last'] = ('bound', np.concatenate([valid, bad]), dict())
    for k in range(len(INVALID_POINTS)):
        cases['invalid_alone%d' % k] = ('bound', bad[k:k + 1], dict())
    cases['bound'] = ('bound', _bound_points()[0], dict())
    cases['tie'] = ('tie', TIE_POINT, dict())
    cases['tie_on_the_gate'] = ('tie', TIE_POINT, dict(max_distance=0.125))
    cases['tie_below_the_gate'] = ('tie', TIE_POINT, dict(max_distance=float(np.nextafter(0.125, 0))))
    # own voxel fails the filter beside a kept one; empty own voxel beside kept ones; nothing within 27 voxels; the lone far voxel itself
    fpts = np.array([[0.09, 0.05, 0.05], [0.22, 0.05, 0.05], [1.0, 1.0, 1.0], [2.05, 2.05, 2.05]], np.float32)
    cases['filter'] = ('filter', fpts, dict(max_moving_fraction=0.0))
    cases['filter_none'] = ('filter', fpts, dict())
    rpts = np.concatenate([ah.centres([v for v, _, _ in RATIO_SPEC], 1.0), ah.centres([v for v, _, _ in RATIO_SPEC], 1.0) + np.float32(0.3)])
    for k, (f, _) in enumerate(RATIO_FILTERS):
        cases['ratio_filter%d' % k] = ('ratio', rpts, dict(f))
    cases['pose'] = ('corner', _corner_scan(), dict(pose=POSE))
    cases['pose_filtered'] = ('corner', _corner_scan(), dict(pose=POSE, max_distance=0.05, **FILTER))
    far = np.array([[5.0, 5.0, 5.0], [np.nan, 1.0, 1.0]], np.float32)
    for tag, extra in (('normals', dict(normals=True)), ('require', dict(normals=True, require_normal=True)),
                       ('normals_filtered', dict(normals=True, viewpoints=np.array([[1.5, -0.2, 1.3]] * 4), **FILTER)),
                       ('require_filtered_r2', dict(normals=True, require_normal=True, radius=2, min_neighbors=8, **FILTER))):
        cases['corner_' + tag] = ('corner', np.concatenate([_corner_scan(), far]), dict(pose=POSE, **extra))
    # flag 1 on purpose: min_neighbors = 9 leaves the sheets' rims without a normal
    cases['corner_few_normals'] = ('corner', _corner_scan(), dict(pose=POSE, normals=True, min_neighbors=9))
    cases['corner_few_require'] = ('corner', _corner_scan(), dict(pose=POSE, normals=True, require_normal=True, min_neighbors=9))
    cases['bad_table'] = ('corner', _corner_scan(), dict(pose=POSE, normals=True, short_rows=1))
    cases['bad_table_require'] = ('corner', _corner_scan(), dict(pose=POSE, normals=True, require_normal=True, short_rows=1, **FILTER))
    cases['plane_normals'] = ('plane', ah.noisy_plane()[::20] + np.float32(0.013), dict(normals=True, max_distance=0.09))
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_query_host_driver', 'query_host')


def _run_host(exe, tmp_path, tag, records, pierced, points, spare=3, pose=None, max_distance=None, voxel_size=0.1, min_count=1, max_moving_fraction=None,
              normals=False, require_normal=False, radius=1, min_neighbors=5, viewpoints=None, stamp_base=0, short_rows=0):
    m, n = records[0].shape[0], points.shape[0]
    view = np.zeros((0, 3)) if viewpoints is None else np.asarray(viewpoints, np.float64).reshape(-1, 3)
    head = [m, m + spare, 0 if pierced is None else 1, min_count, 0 if max_moving_fraction is None else 1, 1 if normals else 0, 1 if require_normal else 0,
            radius, min_neighbors, view.shape[0], stamp_base, n, 0 if pose is None else 1, short_rows]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64),
                        np.array([0.0 if max_moving_fraction is None else max_moving_fraction, voxel_size, voxel_size if max_distance is None else max_distance],
                                 np.float64),
                        ah.map_bytes(*records, pierced), view, np.ascontiguousarray(points, np.float32),
                        b'' if pose is None else np.ascontiguousarray(pose, np.float64))
    kept = int(np.frombuffer(raw, np.int64, 1, 56)[0])
    v = kept if normals else 0
    layout = [('normals32', np.float32, (v, 3)), ('flags', np.uint8, (v,))] + [(f, qref.DTYPES[f], (n, 3) if f == 'nearest' else (n,)) for f in qref.FIELDS]
    out, off = ah.unpack(raw, 64, layout)
    assert off == len(raw)
    return dict(out, counters=np.frombuffer(raw, np.int64, 7).tolist(), kept=kept)


_hosted, _restated = {}, {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, points, args = CASES[name]
        r, pierced = _scene(scene)
        keys = r.records()[0]
        _hosted[name] = _run_host(exe, tmp_path, name, r.records(), None if pierced is None else ah.aligned(pierced, keys), points,
                                  voxel_size=r.voxel_size, **args)
    return _hosted[name]


def _restate(exe, tmp_path, name):
    """The restatement's result of a case, computed once; the float32 normals and flags are the host build's (C5 has its own tests)."""
    if name not in _restated:
        scene, points, args = CASES[name]
        r, pierced = _scene(scene)
        a = {k: args[k] for k in ('pose', 'max_distance', 'min_count', 'max_moving_fraction', 'require_normal') if k in args}
        if args.get('normals'):
            host = _host(exe, tmp_path, name)
            a.update(normals32=host['normals32'], flags=host['flags'], bad_table=args.get('short_rows', 0) > 0)
        _restated[name] = qref.query(r, pierced, points, **a)
    return _restated[name]


def _assert_same(got, want, what):
    assert list(got['counters']) == list(want['counters']), (what, got['counters'], want['counters'])
    for f in qref.FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert np.array_equal(ah.bits(got[f]), ah.bits(want[f])), (what, f, np.flatnonzero(ah.bits(got[f]).reshape(got[f].shape[0], -1) !=
                                                                                         ah.bits(want[f]).reshape(got[f].shape[0], -1))[:5])


# ---- CPU: host build == restatement -------------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    assert [_scene('rows%d' % m)[0].num_voxels for m in (0, 1, 65, 343)] == [0, 1, 65, 343]
    vox, decoys = ah.bound_voxels()
    assert _scene('bound')[0].num_voxels == len(set(vox + decoys)) and len(decoys) >= 36
    corner = _scene('corner')[0]
    assert 1000 < len(qref.kept_voxels(corner, **FILTER)) < corner.num_voxels
    assert abs(np.rad2deg(np.arccos((np.trace(POSE[:3, :3]) - 1) / 2)) - 1.0) < 0.1 and 0.2 < np.linalg.norm(POSE[:3, 3]) / 0.1 < 0.4


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want, got = _restate(host_exe, tmp_path, name), _host(host_exe, tmp_path, name)
    _assert_same(got, want, name)
    s = got['status']
    assert got['counters'][:6] == [len(s)] + [int(((s & b) != 0).sum()) for b in (I, O, K, M, N)]
    un = (s & M) == 0                                                             # the defaults: a threshold distance < x never admits an unmatched point
    assert (got['row'][un] == -1).all() and np.isposinf(got['distance'][un]).all() and (got['nearest'][un] == 0).all()
    assert np.isposinf(got['plane_distance'][(s & N) == 0]).all() and np.isfinite(got['plane_distance'][(s & N) != 0]).all()
    assert (got['distance'][~un] <= CASES[name][2].get('max_distance', _scene(CASES[name][0])[0].voxel_size)).all()


def test_sizes_and_validity(host_exe, tmp_path):
    for n in POINT_COUNTS:
        empty = _host(host_exe, tmp_path, 'n%d_rows0' % n)
        assert empty['counters'] == [n, 0, 0, 0, 0, 0, 0] and (empty['status'] == 0).all()          # m = 0: every valid point gets status 0
        full = _host(host_exe, tmp_path, 'n%d_rows343' % n)
        assert full['counters'][0] == n and (n < 63 or 0 < full['counters'][2] < n) and (n < 63 or full['counters'][4] > 0)
    with_rays, without = _host(host_exe, tmp_path, 'n257_rows343'), _host(host_exe, tmp_path, 'n257_rows343_no_sidecar')
    assert with_rays['pierced'].max() > 0 and (without['pierced'] == 0).all()
    k = len(INVALID_POINTS)
    first, last = _host(host_exe, tmp_path, 'invalid_first'), _host(host_exe, tmp_path, 'invalid_last')
    assert (first['status'][:k] == I).all() and (first['status'][k:] & (I | O | M) == (O | M)).all() and first['counters'][1] == k
    assert (last['status'][-k:] == I).all() and (last['status'][:-k] & (I | O | M) == (O | M)).all()
    for f in qref.FIELDS[1:]:
        assert np.array_equal(ah.bits(first[f][:k]), ah.bits(last[f][-k:])) and np.array_equal(ah.bits(first[f][k:]), ah.bits(last[f][:-k])), f
    for j in range(k):
        assert _host(host_exe, tmp_path, 'invalid_alone%d' % j)['counters'] == [1, 1, 0, 0, 0, 0, 0]


def test_index_bound_and_decoys(host_exe, tmp_path):
    """Points in the last voxel of every axis at both ends: offsets that leave the grid are skipped, and a voxel where an overflowed y / z field would alias
    is never matched -- the matched voxel is always one of the 27 around the point."""
    got = _host(host_exe, tmp_path, 'bound')
    pts, last = _bound_points()
    kept = qref.kept_voxels(_scene('bound')[0])
    assert (got['status'] == (O | K | M)).all() and got['counters'] == [len(pts), 0, len(pts), len(pts), len(pts), 0, 0]
    own = np.array(last + last)
    found = np.array([kept[j][0] for j in got['row'].tolist()])
    assert np.abs(found - own).max() <= 1
    assert np.array_equal(found[:len(last)], own[:len(last)])                      # a voxel centre finds its own voxel


def test_exact_boundaries(host_exe, tmp_path):
    kept = qref.kept_voxels(_scene('tie')[0])
    for name in ('tie', 'tie_on_the_gate'):
        got = _host(host_exe, tmp_path, name)
        # own voxel (1,0,0); both centres at exactly 0.125: the strict < keeps the lowest key, (0,0,0)
        assert got['status'].tolist() == [O | K | M] and kept[int(got['row'][0])][0] == (0, 0, 0) and got['distance'].tolist() == [0.125], name
        assert got['nearest'].tolist() == [[0.125, 0.125, 0.125]]
    below = _host(host_exe, tmp_path, 'tie_below_the_gate')
    assert below['status'].tolist() == [O | K] and below['row'].tolist() == [-1] and np.isposinf(below['distance'][0])


def test_filter_cases(host_exe, tmp_path):
    got = _host(host_exe, tmp_path, 'filter')
    kept = qref.kept_voxels(_scene('filter')[0], max_moving_fraction=0.0)
    assert [c for c, _ in kept] == [(1, 0, 0), (3, 0, 0), (20, 20, 20)]
    assert got['status'].tolist() == [O | M, M, 0, O | K | M] and got['row'].tolist() == [0, 0, -1, 2]
    assert got['count'].tolist() == [3, 0, 0, 1] and got['moving'].tolist() == [1, 0, 0, 0] and got['t_last'].tolist() == [2, 0, 0, 0]
    assert got['pierced'].tolist() == [3, 0, 0, 0]
    assert _host(host_exe, tmp_path, 'filter_none')['status'].tolist() == [O | K | M, M, 0, O | K | M]
    for k, (_, n) in enumerate(RATIO_FILTERS):                                    # filter ratios exactly on a record's ratio
        got = _host(host_exe, tmp_path, 'ratio_filter%d' % k)
        assert got['counters'][2:4] == [14, 2 * n] and int(((got['status'][:7] & K) != 0).sum()) == n, k


def test_normals_and_bad_table(host_exe, tmp_path):
    plain, need = _host(host_exe, tmp_path, 'corner_few_normals'), _host(host_exe, tmp_path, 'corner_few_require')
    flagged = (plain['status'] & (M | N)) == M                                   # matched a row with flag 1: MATCHED without NORMAL ...
    assert flagged.sum() >= 5 and (plain['flags'][plain['row'][flagged]] & 3 != 0).all()
    moved = need['status'][flagged]                                              # ... the next candidate or nothing with require_normal
    assert (((moved & (M | N)) == (M | N)) | ((moved & M) == 0)).all()
    assert (need['distance'][flagged] >= plain['distance'][flagged]).all() and (need['row'][flagged] != plain['row'][flagged]).all()
    assert need['counters'][4] == need['counters'][5] <= plain['counters'][4] and plain['counters'][5] < plain['counters'][4]
    same = ~flagged & ((plain['status'] & N) != 0)
    assert np.array_equal(plain['row'][same], need['row'][same]) and np.array_equal(ah.bits(plain['plane_distance'][same]), ah.bits(need['plane_distance'][same]))
    ok = _host(host_exe, tmp_path, 'corner_normals')
    on = (ok['status'] & N) != 0
    assert on.sum() > 700 and (np.abs(ok['plane_distance'][on]) <= ok['distance'][on] * (1 + 1e-6)).all()
    for name in ('bad_table', 'bad_table_require'):
        bad, good = _host(host_exe, tmp_path, name), _host(host_exe, tmp_path, 'pose' if name == 'bad_table' else 'pose_filtered')
        assert bad['counters'][6] == 1 and bad['counters'][4:6] == [0, 0] and bad['counters'][:4] == good['counters'][:4]
        assert np.array_equal(bad['status'], good['status'] & (I | O | K)) and np.array_equal(bad['count'], good['count'])


BRUTE = [(scene, f) for scene in ('plane', 'corner', 'uniform') for f in (0.9, 0.5, 0.1)]


@pytest.mark.parametrize('scene,fraction', BRUTE)
def test_the_match_is_the_global_nearest_kept_centroid(scene, fraction):
    """The theorem of the contract: for max_distance <= 0.9 voxel_size the 27-voxel search returns the nearest kept centroid of the WHOLE map."""
    r, _ = _scene(scene)
    rs = np.random.RandomState(int(fraction * 10))
    base = {'plane': ah.noisy_plane()[::40], 'corner': ah.corner(13, 60).astype(np.float32), 'uniform': rs.uniform(-0.7, 0.7, (150, 3)).astype(np.float32)}[scene]
    pts = np.concatenate([base + rs.normal(0, 0.04, base.shape).astype(np.float32), [[np.inf, 0, 0]]]).astype(np.float32)
    f = FILTER if scene == 'corner' else dict()
    got = qref.query(r, None, pts, max_distance=fraction * 0.1, **f)
    valid, row, dist = qref.brute_force(r, pts, max_distance=fraction * 0.1, **f)
    assert np.array_equal(valid, got['status'] != I) and valid.sum() == len(pts) - 1
    assert np.array_equal(row[valid], got['row'][valid]) and np.array_equal(ah.bits(dist[valid]), ah.bits(got['distance'][valid]))
    assert (fraction < 0.2 or (row >= 0).sum() > 0) and (fraction > 0.2 or (row < 0).sum() > 0)


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_query_workspace_bytes', 'pcacc_accum_query'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C9. ' in header and len(native._PROTOTYPES['pcacc_accum_query']) == 32
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_query.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_register.h"']
    for helper in ('accr_world(', 'accr_match(', 'accn_centroid', 'accum_field(', 'accum_lower_bound(', 'accn_index(', 'accum_keep('):
        assert helper in text, helper
    assert (native.QUERY_INVALID, native.QUERY_OCCUPIED, native.QUERY_KEPT, native.QUERY_MATCHED, native.QUERY_NORMAL, native.QUERY_COUNTERS) == (1, 2, 4, 8, 16, 7)
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.query(torch.zeros(4, 3))
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).query(np.zeros((4, 3), np.float32))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def _device_cloud(r, pierced):
    """The restatement's map and {coord: rays} dict as an AccumulatedCloud on the device."""
    return ah.device_cloud(r, None if pierced is None else ah.aligned(pierced, r.records()[0]), np.zeros(5, np.int64))


_clouds = {}


def _cloud(scene):
    """A device map per scene, shared: query does not modify it (a test below says so)."""
    if scene not in _clouds:
        _clouds[scene] = _device_cloud(*_scene(scene))
    return _clouds[scene]


def _query(m, points, args):
    from pcaccumulation_amd import native
    a = dict(args)
    short = a.pop('short_rows', 0)
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(DEV)
    if not short:
        return m.query(pts, **a)
    nrm = m.normals(a.get('radius', 1), a.get('min_neighbors', 5), a.get('min_count', 1), a.get('max_moving_fraction'), a.get('viewpoints'))
    v = nrm['flags'].shape[0] - short                                             # tables short by a row: values the host knows
    return native.accum_query(pts, m._pose(a.get('pose')), m.voxel_size, a.get('max_distance', m.voxel_size), m._cur, m.num_voxels, m._pierced,
                              a.get('min_count', 1), a.get('max_moving_fraction'), nrm['normals'][:v].contiguous(), nrm['flags'][:v].contiguous(),
                              a.get('require_normal', False))


def _assert_device_equals_host(res, host, what):
    assert sorted(res) == sorted(qref.FIELDS + ('counters',))
    assert res['counters'].dtype == torch.int64 and res['counters'].tolist() == host['counters'], (what, res['counters'].tolist(), host['counters'])
    for f in qref.FIELDS:
        want = torch.from_numpy(host[f]).to(DEV)
        assert res[f].is_cuda and res[f].dtype == want.dtype and res[f].shape == want.shape, (what, f)
        if want.dtype.is_floating_point:                                            # torch.equal on the bits: +inf, -0.0 and every last bit
            assert torch.equal(res[f].view(torch.int64 if want.dtype == torch.float64 else torch.int32), torch.from_numpy(ah.bits(host[f])).to(DEV)), (what, f)
        assert torch.equal(res[f], want), (what, f)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    scene, points, args = CASES[name]
    host = _host(host_exe, tmp_path, name)
    m = _cloud(scene)
    snap = ah.snapshot(m, whole_sidecar=True)
    res = _query(m, points, args)
    _assert_device_equals_host(res, host, name)
    again = _query(m, points, args)                                               # a second run gives the same bits
    assert all(torch.equal(res[f], again[f]) for f in res)
    ah.assert_unchanged(m, snap, name)                                              # read-only: keys, records, stamps, sidecar, state words, num_voxels


@pytest.mark.gpu
@pytest.mark.parametrize('args', [dict(max_distance=0.07), dict(normals=True, require_normal=True, pose=ah.rot_xyz(0.002, -0.001, 0.003, (0.01, 0.02, -0.01)))],
                         ids=['plain', 'normals_pose'])
def test_kernel_on_76661_voxels_and_100003_points_gpu(host_exe, tmp_path, args):
    r, _ = _scene('wavy')
    rs = np.random.RandomState(77)
    pts = ah.wavy()[rs.randint(0, 270400, 100003)] + rs.uniform(-0.03, 0.03, (100003, 3)).astype(np.float32)
    pts[::3, 2] += rs.uniform(0.0, 0.2, pts[::3].shape[0]).astype(np.float32)      # a third lifted off the sheet by up to two voxels
    assert r.num_voxels == 76661 and pts.shape[0] % 64 != 0 and pts.shape[0] % 256 != 0
    host = _run_host(host_exe, tmp_path, 'wavy', r.records(), None, pts, **args)
    m = _cloud('wavy')
    res = _query(m, pts, args)
    _assert_device_equals_host(res, host, 'wavy')
    assert 0 < host['counters'][4] < host['counters'][0] and host['counters'][2] > 20000
    assert all(torch.equal(res[f], v) for f, v in _query(m, pts, args).items())


@pytest.mark.gpu
def test_identities_with_extract_and_pierced_gpu():
    from pcaccumulation_amd import native
    r, _ = _scene('corner')
    m = _device_cloud(r, {c: (c[0] + c[1]) % 3 for c, _ in qref.kept_voxels(r)})
    for f in (dict(), FILTER):
        e, seen = m.extract(**f), m.pierced(**f)
        v = e['points'].shape[0]
        # the restatement says so for this scene: every centroid finds itself, none is nearer to another voxel's centroid
        own = qref.query(r, None, e['points'].cpu().numpy(), **f)
        assert np.array_equal(own['row'], np.arange(v)) and (own['distance'] <= 2.0 ** -18).all()
        got = m.query(e['points'], **f)
        assert bool(((got['status'] & M) != 0).all()) and float(got['distance'].max()) <= 2.0 ** -18
        assert torch.equal(got['row'], torch.arange(v, dtype=torch.int32, device=DEV)) and torch.equal(got['nearest'], e['points'])
        scan = torch.from_numpy(np.concatenate([_corner_scan(), [[9.0, 9.0, 9.0], [np.nan, 0, 0]]]).astype(np.float32)).to(DEV)
        got = m.query(scan, pose=POSE, **f)
        s = got['status']
        matched, kept = (s & M) != 0, (s & K) != 0
        assert 0 < int(matched.sum()) < scan.shape[0] and 0 < int(kept.sum())
        assert torch.equal(e['points'][got['row'][matched].long()], got['nearest'][matched])
        # a coordinate join: the point's voxel (float64, the map's own division) -> its row of extract
        p, T = scan[kept].double(), POSE
        w = torch.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1)   # the contract's order, element-wise
        idx = torch.floor(w / m.voxel_size).long() + native.ACCUM_IDX_BIAS
        c = e['coords'].long() + native.ACCUM_IDX_BIAS
        join = torch.searchsorted((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2])
        assert torch.equal(e['coords'][join].long(), idx - native.ACCUM_IDX_BIAS)
        for name in ('count', 'moving', 't_first', 't_last'):
            assert torch.equal(got[name][kept], e[name][join]), name
        assert torch.equal(got['pierced'][kept], seen[join]) and int(got['pierced'].max()) == 2
        assert got['counters'].tolist() == [scan.shape[0]] + [int(((s & b) != 0).sum()) for b in (I, O, K, M, N)] + [0]


@pytest.mark.gpu
def test_tie_to_register_gpu():
    m = _cloud('corner')
    scan = torch.from_numpy(_corner_scan(1300)).to(DEV)
    for f in (dict(), FILTER):
        q = m.query(scan, pose=POSE, normals=True, require_normal=True, max_distance=0.08, **f)
        reg = m.register(scan, init_pose=POSE, max_iter=0, max_distance=0.08, **f)
        n_matched = int(q['counters'][4])
        assert int(reg['correspondences']) == int(q['counters'][5]) == n_matched > 1000
        assert float(reg['fitness']) == n_matched / scan.shape[0]
        r = q['plane_distance'][(q['status'] & M) != 0]
        rmse = float(torch.sqrt((r * r).mean()))
        print('rmse: register %.17g, query %.17g' % (float(reg['rmse']), rmse))
        assert abs(rmse - float(reg['rmse'])) <= 1e-9 * float(reg['rmse'])       # the two sums run in different orders: n 2^-53 < 1.2e-10 for n < 2^20


def _both_add(m, r, pts, stamp, pose=None):
    m.add(torch.from_numpy(pts).to(DEV), pose, stamp=stamp)
    r.add(pts, pose, stamp=stamp)


def _both_see(m, r, pierced, pts, origin, stamp):
    m.see_through(torch.from_numpy(pts).to(DEV), origin, stamp=stamp)
    pref.pierce(pref.voxels_of(r), pts, origin, voxel_size=r.voxel_size, stamp=stamp, pierced=pierced)


def _assert_query_equals_restatement(m, r, pierced, pts, what, **args):
    got = m.query(torch.from_numpy(pts).to(DEV), **args)
    want = qref.query(r, pierced, pts, **args)
    _assert_same({k: (v.tolist() if k == 'counters' else v.cpu().numpy()) for k, v in got.items()}, want, what)
    e = m.extract(args.get('min_count', 1), args.get('max_moving_fraction'))      # `row` refers to the rows of the extract of that moment
    matched = (got['status'] & M) != 0
    assert torch.equal(e['points'][got['row'][matched].long()], got['nearest'][matched]), what
    return got


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, pierced = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), {}
    origin = np.array([[0.05, 0.05, 0.05]])
    slab = ah.centres([(x, y, z) for x in (5, 6, 7) for y in range(-2, 3) for z in (-1, 0, 1)], 0.1)
    probe = np.concatenate([slab + np.float32(0.03), ah.centres([(9, 0, 0), (6, 9, 9), (-9, 0, 0)], 0.1), [[np.nan, 0, 0]]]).astype(np.float32)
    _both_add(m, r, np.concatenate([slab, slab[::2]]), 0)
    a = _assert_query_equals_restatement(m, r, None, probe, 'after add', min_count=2)
    _both_see(m, r, pierced, ah.centres([(20, y, 0) for y in (-2, 0, 3)], 0.1), origin, 1)
    b = _assert_query_equals_restatement(m, r, pierced, probe, 'after see_through', min_count=2)
    assert int(a['pierced'].sum()) == 0 < int(b['pierced'].sum()) and torch.equal(a['row'], b['row'])
    assert m.prune(min_pierced=1)['pierced'] == rref.prune(r, pierced, min_pierced=1)[4] > 0
    c = _assert_query_equals_restatement(m, r, pierced, probe, 'after prune', min_count=2)
    assert int(c['counters'][2]) < int(b['counters'][2]) and int(c['pierced'].sum()) == 0
    _both_add(m, r, ah.centres([(-9, 0, 0), (6, 0, 0), (6, 0, 0), (6, 9, 9)], 0.1), 2)
    d = _assert_query_equals_restatement(m, r, pierced, probe, 'add after prune')
    assert int(d['counters'][2]) > int(c['counters'][2])
    path = os.path.join(str(tmp_path), 'map.npz')
    m.save(path)
    loaded = AccumulatedCloud.load(path, DEV)
    e = _assert_query_equals_restatement(loaded, r, pierced, probe, 'after load')
    assert all(torch.equal(d[f], e[f]) for f in d)


# ---- the ghost scene of section 9f, rebuilt here --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ghost_trail_seen_from_a_fresh_scan_gpu():
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, pierced = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), {}
    scans = ah.ghost_scans()
    for k, (wall, cluster, _) in enumerate(scans):
        pts = np.concatenate([wall, cluster])
        _both_see(m, r, pierced, pts, ah.GHOST_SENSOR, k)
        _both_add(m, r, pts, k)
    rs = np.random.RandomState(8)
    wall_vox = [(30, int(y), int(z)) for y, z in zip(rs.randint(-20, 20, 400), rs.randint(-10, 10, 400))]
    early = sorted({v for k in range(5) for v in scans[k][2]})
    ghost_vox = [early[i] for i in rs.permutation(len(early))[:100]]
    free_vox = [(8, int(y), int(z)) for y, z in zip(rs.randint(-20, 20, 100), rs.randint(-10, 10, 100))]
    fresh = (ah.centres(wall_vox + ghost_vox + free_vox, 0.1) + rs.uniform(-0.04, 0.04, (600, 3)).astype(np.float32)).astype(np.float32)
    got = _assert_query_equals_restatement(m, r, pierced, fresh, 'ghost before')
    s, p = got['status'].cpu().numpy(), got['pierced'].cpu().numpy()
    assert ((s[:400] & K) != 0).all() and (p[:400] == 0).all()                   # the wall: kept, no ray went through it
    with_rays = np.array([pierced.get(v, 0) >= 1 and rref.key_of(v) in r.rec for v in ghost_vox])
    assert with_rays.sum() >= 50 and (p[400:500][with_rays] >= 1).all()           # the trail: occupied, and rays went through it
    assert ((s[500:] & O) == 0).all()                                             # free space: nothing has been seen there
    res = m.prune(min_pierced=1)
    assert [res[f] for f in rref.NAMES] == rref.prune(r, pierced, min_pierced=1)
    after = _assert_query_equals_restatement(m, r, pierced, fresh, 'ghost after')
    s2 = after['status'].cpu().numpy()
    lost = np.array([rref.key_of(v) not in r.rec for v in ghost_vox])
    assert lost.sum() >= 50 and ((s2[400:500][lost] & O) == 0).all() and ((s2[:400] & K) != 0).all()
    assert after['counters'].tolist() == qref.query(r, pierced, fresh)['counters']


@pytest.mark.gpu
def test_novelty_of_drifting_windows_gpu():
    """Eight windows of the corner seen from a moving sensor.  counters[occupied] per window equals the restatement's, and a window added with a drifted
    pose leaves more of the next look at the same window unexplained than the window added with the registered pose."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1)
    occupied = []
    for k in range(8):
        truth = ah.rot_xyz(0.002 * k, -0.001 * k, 0.003 * k, (0.05 * k, -0.03 * k, 0.01 * k))
        inv = np.linalg.inv(truth)
        pts = (ah.corner(40 + k, 250) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        if k:
            got = m.query(torch.from_numpy(pts).to(DEV), pose=truth)
            want = qref.query(r, None, pts, pose=truth)
            assert got['counters'].tolist() == want['counters']
            occupied.append(want['counters'][2])
        _both_add(m, r, pts, k, truth)
    assert all(o > 300 for o in occupied)
    # the same window, added once with a drifted pose (1.5 voxels off) and once with the pose a registration returns
    truth = ah.rot_xyz(0.016, -0.008, 0.024, (0.4, -0.24, 0.08))
    inv = np.linalg.inv(truth)
    window = torch.from_numpy((ah.corner(48, 250) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)).to(DEV)
    again = torch.from_numpy((ah.corner(49, 250) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)).to(DEV)
    drifted = truth.copy()
    drifted[:3, 3] += (0.15, -0.15, 0.15)
    started = truth.copy()
    started[:3, 3] += (0.03, -0.02, 0.02)
    reg = m.register(window, init_pose=started, max_iter=20)
    assert int(reg['status']) in (0, 16)
    count = {tag: int(m.query(window, pose=pose)['counters'][2]) for tag, pose in (('drifted', drifted), ('registered', reg['pose']))}
    print('occupied per window %s; the ninth window under the drifted pose %d, under the registered pose %d of 750' % (occupied, count['drifted'], count['registered']))
    assert count['drifted'] < count['registered']
    assert int(m.query(again, pose=truth)['counters'][0]) == 750


@pytest.mark.gpu
def test_query_results_on_the_model_forward_gpu(golden):
    """query_results on the model_tiny_test forward runs, the counters sum correctly and status has no bit above 16.  Nothing more is claimed."""
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
    res = m.query_results(out, inp, pose=ah.rot_xyz(0, 0, 0.01, (0.02, -0.01, 0.0)), normals=True)
    same = m.query(out['rec_est'], ah.rot_xyz(0, 0, 0.01, (0.02, -0.01, 0.0)), normals=True)
    assert all(torch.equal(res[k], same[k]) for k in res)
    s = res['status']
    n = out['rec_est'].shape[0]
    assert int(s.max()) < 32 and res['counters'].tolist() == [n] + [int(((s & b) != 0).sum()) for b in (I, O, K, M, N)] + [0]
    assert int(res['counters'][2]) > 0
    with pytest.raises(ValueError):
        m.query_results(dict(out, _n_batches=2), inp)


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    r, pierced = _scene('rows65')
    m = _device_cloud(r, pierced)
    snap = ah.snapshot(m, whole_sidecar=True)
    n = 10
    pts = torch.from_numpy(_block_points(n, 1)).to(DEV)
    out = {name: torch.full((n,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in native.QUERY_FIELDS}
    counters = torch.full((7,), 7, dtype=torch.int64, device=DEV)
    nrm = m.normals()
    v = nrm['flags'].shape[0]
    good = dict(points=pts, pose=None, voxel_size=0.1, max_distance=0.1, tables=m._cur, m=65, pierced=m._pierced, min_count=1, max_moving_fraction=None,
                normals=nrm['normals'], flags=nrm['flags'], require_normal=False, out=out, counters=counters)
    for bad in (dict(m=-1), dict(m=m.capacity + 1), dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float('inf')), dict(voxel_size=float('nan')),
                dict(max_distance=0.0), dict(max_distance=-0.05), dict(max_distance=0.1000001), dict(max_distance=float('nan')),
                dict(flags=None), dict(normals=None), dict(normals=None, flags=None, require_normal=True),
                dict(m=v - 1)):                                                    # n_rows = v > m
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_query(**dict(good, **bad))
    lib = native.lib()
    ptr = [native._dev(out[name]) for name, _, _ in native.QUERY_FIELDS]
    keys, acc, stamps = (native._dev(t) for t in m._cur)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def call(n_points=n, points=native._dev(pts), ptr=ptr, keys=keys, cnt=native._dev(counters), ws_bytes=ws.numel(), n_rows=0):
        return lib.pcacc_accum_query(points, n_points, None, 0.1, 0.1, keys, acc, stamps, None, m.capacity, 65, 1, 0, 0.0, None, None, n_rows, 0, *ptr, cnt,
                                     native._dev(ws), ws_bytes, native._stream())
    assert call(n_points=-1) == call(n_points=(1 << 30) + 1) == call(points=None) == call(keys=None) == call(cnt=None) == call(ws_bytes=16) == -1
    assert call(n_rows=3) == -1                                                   # rows without tables
    for k in range(len(ptr)):
        assert call(ptr=ptr[:k] + [None] + ptr[k + 1:]) == -1, k                  # a NULL output of non-zero size
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in list(out.values()) + [counters])     # nothing was launched: outputs and counters keep their poison
    ah.assert_unchanged(m, snap, 'bad arguments')
    for bad in (dict(max_distance=0.0), dict(max_distance=0.1000001), dict(max_distance=float('nan')), dict(radius=0), dict(radius=4), dict(min_neighbors=2),
                dict(require_normal=True), dict(pose=np.eye(3))):
        with pytest.raises(ValueError):
            m.query(pts, **bad)
    with pytest.raises(ValueError):
        m.query(pts[:, :2])
    with pytest.raises(native.NativeError):
        m.query(pts.cpu())
    zero = native.accum_query(**dict(good, points=pts[:0], out={k: t[:0] for k, t in out.items()}))      # n = 0: the zero counters and nothing else
    assert zero['counters'].tolist() == [0] * 7 and all(bool((t == 7).all()) for t in out.values())
    assert call() == 0 and counters.tolist()[0] == n and not bool((out['status'] == 7).any())
    ah.assert_unchanged(m, snap, 'after all')
