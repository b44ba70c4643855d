"""The k nearest kept centroids of the accumulated scene cloud within a few voxels (include/pcacc.h C16): AccumulatedCloud.knn /
knn_results / neighbors / outliers.

Every result is an integer or a float64 computed by + - * / and sqrt in one order, and the (d2, row) order of a result is total, so every claim is an
equality of bits:
  CPU   the g++ build of csrc/accum_knn.h (tests/accum_knn_host_driver.cpp, every table index asserted, poison behind the rows in use and in every output,
        every output row written once) against the plain-Python restatement on coordinate dicts (tests/accumulate_knn_reference.py: no keys, no sort of
        the map, no running top-k), and the restatement against a brute force over ALL kept centroids for max_distance <= (r - 0.1) voxel_size;
  GPU   both kernels against the g++ build on the same cases, then identities that tie knn to query and to extract, a symmetry of the self mode, a life
        cycle against the restatement and the outlier removal of a plane with floaters.
The one tolerance (1e-9 relative) is the outlier threshold, a mean and a standard deviation whose sums run in another order than numpy's: n 2^-53 <
1.2e-10 for n < 2^20, register's bound for its rmse."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_knn_reference as kref
import accumulate_prune_reference as rref
import accumulate_query_reference as qref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

I, F, U = kref.INVALID, kref.FOUND, kref.FULL
FILTER = dict(min_count=2, max_moving_fraction=0.5)
POSE = ah.rot_xyz(np.deg2rad(0.6), np.deg2rad(-0.5), np.deg2rad(0.7), (0.02, -0.015, 0.017))      # C9's: about 1 degree and 0.3 voxel of 0.1 m


# ---- scenes: a ReferenceMap each, built once and never modified ------------------------------------------------------------------------------------------
def _corner_adds():
    """C9's corner scene: three noisy sheets, some points flagged moving, two stamps."""
    pts = ah.corner(11, 3000).astype(np.float32)
    mv = (pts[:, 0] > ah.CORNER[0] + 1.6) & (np.random.RandomState(4).uniform(0, 1, pts.shape[0]) < 0.5)
    return [(pts[:5000], mv[:5000], 3), (pts[5000:], mv[5000:], 1)]


def _outlier_points():
    """A 24 x 24 voxel sheet of 0.1 m voxels, one point per voxel with 2 cm of noise about the voxel centre, and five floaters 0.25 - 0.55 m above it,
    each alone in its neighbourhood.  The floaters are the LAST five voxels in no order: their rows are found by coordinate."""
    rs = np.random.RandomState(31)
    g = np.arange(-12, 12)
    x, y = np.meshgrid(g, g, indexing='ij')
    sheet = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)
    pts = (sheet + 0.5) * 0.1 + rs.uniform(-0.02, 0.02, (x.size, 3))
    return pts.astype(np.float32), ah.centres(FLOATERS, 0.1)


# k = 4 and three standard deviations: the rows on the rim of a finite sheet have neighbours on one side only and a larger mean distance than the rows inside
# (0.132 m against 0.10 m); the threshold comes to 0.150 m, the nearest floater has 0.210 m
OUTLIER_ARGS = dict(k=4, std_ratio=3.0, radius=4)
FLOATERS = [(-8, -7, 2), (-1, 6, 3), (3, -4, 2), (8, 8, 5), (9, -9, 3)]

_scenes = {}


def _build_scene(name):
    if name.startswith('rows'):
        return ah.records(0.1, ah.random_rows(int(name[4:]), 100 + int(name[4:]))[0])
    if name == 'dense11':                                                          # 1331 voxels, centroids anywhere inside: 729 candidates per query at r = 4
        return ah.rows([tuple(int(v) for v in c) for c in ah.block(-5, 6)], 3)[0]
    if name == 'tie':                                                              # 0.25 is exact: every centroid exactly at its voxel centre
        return ah.records(0.25, {(x, y, z): (1, 0, 0, 0) for x in (0, 1) for y in (0, 1) for z in (0, 1)})
    if name == 'bound':
        vox, decoys = ah.bound_voxels()
        return ah.points_map(0.01, [(ah.centres(vox + decoys, 0.01), None, 0)])
    if name == 'corner':
        return ah.points_map(0.1, _corner_adds())
    if name == 'uniform':
        return ah.points_map(0.1, [(np.random.RandomState(5).uniform(-0.6, 0.6, (2500, 3)).astype(np.float32), None, 0)])
    assert name == 'outlier'
    return ah.points_map(0.1, [(np.concatenate(_outlier_points()), None, 0)])


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene, the points (None: self mode) and the arguments of one search -------------------------------------------------------------------------
POINT_COUNTS = (0, 1, 63, 64, 65, 257)
KS, RADII = (1, 2, 5, 16), (1, 2, 4)
INVALID_POINTS = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [32768.0, 0, 0], [0, -32768.0, 0], [10486.0, 0, 0], [0, 0, -10486.0]]   # C9's
# equidistant from 2, 4 and 8 of the tie scene's centroids (0.125 and 0.375 on every axis)
TIE_POINTS = np.array([[0.25, 0.125, 0.125], [0.25, 0.25, 0.125], [0.25, 0.25, 0.25]], np.float32)
# extract's rows are (x, y, z) ascending: row = 4 x + 2 y + z.  Per point: the rings of equal distance, inside a ring the lower row first
TIE_ROWS = [[0, 4, 1, 2, 5, 6, 3, 7], [0, 2, 4, 6, 1, 3, 5, 7], [0, 1, 2, 3, 4, 5, 6, 7]]


def _block_points(n, seed, lo=-0.42, hi=0.52):
    """n points over the 7^3 block (11^3 with lo, hi = -0.62, 0.72) and a voxel beyond it on every side."""
    return np.random.RandomState(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def _bound_points():
    vox, _ = ah.bound_voxels()
    last = [v for v in vox if any(c in (-EDGE, EDGE - 1) for c in v)]                # the last voxel of each axis at both ends
    rs = np.random.RandomState(3)
    return np.concatenate([ah.centres(last, 0.01), ah.centres(last, 0.01) + rs.uniform(-0.002, 0.002, (len(last), 3)).astype(np.float32)]), last


def _cases():
    cases = {}
    for n in POINT_COUNTS:
        for scene in ('rows0', 'rows1', 'rows65', 'rows343'):
            cases['n%d_%s' % (n, scene)] = (scene, _block_points(n, n + 1), dict(k=5, radius=2, max_distance=0.19))
    for k in KS:
        for r in RADII:
            cases['k%d_r%d_rows343' % (k, r)] = ('rows343', _block_points(65, 10 * k + r), dict(k=k, radius=r))
            cases['k%d_r%d_dense11' % (k, r)] = ('dense11', _block_points(65, 20 * k + r, -0.62, 0.72), dict(k=k, radius=r))   # r = 4: the replacement path
            cases['self_k%d_r%d_rows343' % (k, r)] = ('rows343', None, dict(k=k, radius=r))
    cases['k16_r4_dense11_reach'] = ('dense11', _block_points(65, 7, -0.62, 0.72), dict(k=16, radius=4, max_distance=0.39))
    cases['n257_rows343_filtered'] = ('rows343', _block_points(257, 9), dict(k=5, radius=2, **FILTER))
    cases['pose'] = ('corner', (ah.corner(12, 100) @ np.linalg.inv(POSE)[:3, :3].T + np.linalg.inv(POSE)[:3, 3]).astype(np.float32),
                     dict(k=8, radius=2, pose=POSE, max_distance=0.15, min_count=2))
    valid = _bound_points()[0][:20]
    bad = np.array(INVALID_POINTS, np.float32)
    cases['invalid_first'] = ('bound', np.concatenate([bad, valid]), dict(k=5, radius=2))
    cases['invalid_last'] = ('bound', np.concatenate([valid, bad]), dict(k=5, radius=2))
    for j in range(len(INVALID_POINTS)):
        cases['invalid_alone%d' % j] = ('bound', bad[j:j + 1], dict(k=5, radius=2))
    for r in (1, 4):
        cases['bound_r%d' % r] = ('bound', _bound_points()[0], dict(k=16, radius=r))
        cases['self_bound_r%d' % r] = ('bound', None, dict(k=16, radius=r))
    cases['tie'] = ('tie', TIE_POINTS, dict(k=8, radius=2))
    cases['tie_padded'] = ('tie', TIE_POINTS, dict(k=16, radius=2))                  # k above the eight candidates
    cases['tie_on_the_gate'] = ('tie', TIE_POINTS, dict(k=8, radius=2, max_distance=0.125))
    cases['tie_below_the_gate'] = ('tie', TIE_POINTS, dict(k=8, radius=2, max_distance=float(np.nextafter(0.125, 0))))
    cases['self_tie'] = ('tie', None, dict(k=16, radius=2))
    for m in (0, 1, 65):
        cases['self_rows%d' % m] = ('rows%d' % m, None, dict(k=5, radius=2))
    cases['self_k16_r4_dense11'] = ('dense11', None, dict(k=16, radius=4))
    cases['self_k8_r2_dense11_reach'] = ('dense11', None, dict(k=8, radius=2, max_distance=0.19))
    cases['self_rows343_filtered'] = ('rows343', None, dict(k=5, radius=2, **FILTER))
    cases['self_rows343_all_filtered'] = ('rows343', None, dict(k=5, radius=2, min_count=7))     # random_rows counts 1..6
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_knn_host_driver', 'knn_host')


def _run_host(exe, tmp_path, tag, r, points, k, radius=2, max_distance=None, pose=None, min_count=1, max_moving_fraction=None, spare=3):
    keys, acc, _ = r.records()
    m, self_mode = keys.shape[0], points is None
    n = 0 if self_mode else points.shape[0]
    head = [m, m + spare, min_count, 0 if max_moving_fraction is None else 1, n, 0 if pose is None else 1, k, radius, 1 if self_mode else 0]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64),
                        np.array([0.0 if max_moving_fraction is None else max_moving_fraction, r.voxel_size,
                                  radius * r.voxel_size if max_distance is None else max_distance], np.float64),
                        ah.map_bytes(keys, acc), np.zeros((0, 3), np.float32) if self_mode else np.ascontiguousarray(points, np.float32),
                        b'' if pose is None else np.ascontiguousarray(pose, np.float64))
    kept, rows = (int(v) for v in np.frombuffer(raw, np.int64, 2, 40))
    assert rows == (kept if self_mode else n)
    fields = kref.SELF_FIELDS if self_mode else kref.FIELDS
    out, off = ah.unpack(raw, 56, [(f, kref.DTYPES[f], (rows, k) if f in ('rows', 'distance') else (rows,)) for f in fields])
    assert off == len(raw)
    return dict(out, counters=np.frombuffer(raw, np.int64, 5).tolist(), kept=kept)


_hosted, _restated = {}, {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, points, args = CASES[name]
        _hosted[name] = _run_host(exe, tmp_path, name, _scene(scene), points, **args)
    return _hosted[name]


def _restate(name):
    if name not in _restated:
        scene, points, args = CASES[name]
        _restated[name] = kref.neighbors(_scene(scene), **args) if points is None else kref.knn(_scene(scene), points, **args)
    return _restated[name]


def _assert_same(got, want, what):
    assert list(got['counters']) == list(want['counters']), (what, got['counters'], want['counters'])
    fields = [f for f in kref.SELF_FIELDS if f in want]
    assert [f for f in kref.SELF_FIELDS if f in got] == fields, what
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(ah.bits(got[f]), ah.bits(want[f])), (what, f, np.flatnonzero((ah.bits(got[f]) != ah.bits(want[f])).reshape(got[f].shape[0], -1).any(1))[:5])


# ---- CPU: host build == restatement == brute force ----------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    assert [_scene('rows%d' % m).num_voxels for m in (0, 1, 65, 343)] == [0, 1, 65, 343] and _scene('dense11').num_voxels == 1331
    assert len(qref.kept_voxels(_scene('rows343'), min_count=7)) == 0 < len(qref.kept_voxels(_scene('rows343'), **FILTER)) < 343
    vox, decoys = ah.bound_voxels()
    assert _scene('bound').num_voxels == len(set(vox + decoys)) and len(decoys) >= 36
    assert [c for c, _ in qref.kept_voxels(_scene('tie'))] == [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want, got = _restate(name), _host(host_exe, tmp_path, name)
    _assert_same(got, want, name)
    scene, points, args = CASES[name]
    k, s, found = args['k'], got['status'], got['found']
    assert got['counters'] == [len(s), int(((s & I) != 0).sum()), int((found > 0).sum()), int((found == k).sum()), int(found.sum())]
    pad = np.arange(k)[None, :] >= found[:, None]                                    # the padding: -1 / +inf behind the found neighbours, nowhere else
    assert np.array_equal(got['rows'] < 0, pad) and np.array_equal(np.isposinf(got['distance']), pad)
    reach = args.get('max_distance', args['radius'] * _scene(scene).voxel_size)
    assert (got['distance'][~pad] <= reach).all() and (got['distance'][:, :-1] <= got['distance'][:, 1:]).all()      # ascending; +inf <= +inf behind
    assert (got['rows'] < got['kept']).all() and np.array_equal(s, np.where(found > 0, F, 0) | np.where(found == k, U, 0) | (s & I))
    if points is None:
        assert got['found'].shape == (got['kept'],) and not (got['rows'] == np.arange(got['kept'])[:, None]).any()     # never itself
        assert np.array_equal(np.isposinf(got['mean_distance']), found == 0)


def test_sizes_validity_and_padding(host_exe, tmp_path):
    for n in POINT_COUNTS:
        empty = _host(host_exe, tmp_path, 'n%d_rows0' % n)
        assert empty['counters'] == [n, 0, 0, 0, 0] and (empty['rows'] == -1).all() and np.isposinf(empty['distance']).all()    # m = 0: all padding
        full = _host(host_exe, tmp_path, 'n%d_rows343' % n)
        assert full['counters'][0] == n and (n < 63 or 0 < full['counters'][3] <= full['counters'][2] <= n)
    k = len(INVALID_POINTS)
    first, last = _host(host_exe, tmp_path, 'invalid_first'), _host(host_exe, tmp_path, 'invalid_last')
    assert (first['status'][:k] == I).all() and (first['status'][k:] & (I | F) == F).all() and first['counters'][1] == k
    assert (first['found'][:k] == 0).all() and (first['rows'][:k] == -1).all() and np.isposinf(first['distance'][:k]).all()
    for f in kref.FIELDS:
        assert np.array_equal(ah.bits(first[f][:k]), ah.bits(last[f][-k:])) and np.array_equal(ah.bits(first[f][k:]), ah.bits(last[f][:-k])), f
    for j in range(k):
        assert _host(host_exe, tmp_path, 'invalid_alone%d' % j)['counters'] == [1, 1, 0, 0, 0]
    assert _host(host_exe, tmp_path, 'self_rows0')['counters'] == [0] * 5 and _host(host_exe, tmp_path, 'self_rows343_all_filtered')['kept'] == 0
    alone = _host(host_exe, tmp_path, 'self_rows1')
    assert alone['counters'] == [1, 0, 0, 0, 0] and np.isposinf(alone['mean_distance']).all()
    dense = _host(host_exe, tmp_path, 'self_k16_r4_dense11')
    assert dense['counters'] == [1331, 0, 1331, 1331, 16 * 1331]                     # 729 candidates, 16 kept: the replacement path


def test_ties_gates_and_padding(host_exe, tmp_path):
    """Exact ties go to the lower row; a neighbour exactly at max_distance is accepted, one ulp below it is not."""
    got = _host(host_exe, tmp_path, 'tie')
    assert got['rows'].tolist() == TIE_ROWS and got['found'].tolist() == [8, 8, 8] and got['status'].tolist() == [F | U] * 3
    ring = [0.125, float(np.sqrt(0.078125)), float(np.sqrt(0.140625))]
    assert got['distance'][0].tolist() == [ring[0]] * 2 + [ring[1]] * 4 + [ring[2]] * 2
    padded = _host(host_exe, tmp_path, 'tie_padded')
    assert padded['rows'][:, :8].tolist() == TIE_ROWS and (padded['rows'][:, 8:] == -1).all() and padded['status'].tolist() == [F] * 3
    assert np.array_equal(ah.bits(padded['distance'][:, :8]), ah.bits(got['distance'])) and np.isposinf(padded['distance'][:, 8:]).all()
    on = _host(host_exe, tmp_path, 'tie_on_the_gate')
    assert on['found'].tolist() == [2, 0, 0] and on['rows'][0].tolist() == [0, 4] + [-1] * 6 and on['distance'][0, :2].tolist() == [0.125, 0.125]
    assert _host(host_exe, tmp_path, 'tie_below_the_gate')['found'].tolist() == [0, 0, 0]
    own = _host(host_exe, tmp_path, 'self_tie')                                      # every centroid: its 3 + 3 + 1 fellows, itself left out
    assert own['found'].tolist() == [7] * 8 and own['rows'][0].tolist() == [1, 2, 4, 3, 5, 6, 7] + [-1] * 9
    assert own['mean_distance'][0] == ((((((0.25 + 0.25) + 0.25) + np.sqrt(0.125)) + np.sqrt(0.125)) + np.sqrt(0.125)) + np.sqrt(0.1875)) / 7.0


def test_index_bound_and_decoys(host_exe, tmp_path):
    """Queries in the last voxel of every axis at both ends: columns outside the grid contribute nothing, and a voxel where an overflowed y / z field
    would alias is never found -- every neighbour lies within `radius` voxels of the query's voxel."""
    kept = qref.kept_voxels(_scene('bound'))
    pts, last = _bound_points()
    for r in (1, 4):
        got = _host(host_exe, tmp_path, 'bound_r%d' % r)
        own = np.array(last + last)
        assert (got['found'] >= (1 if r == 1 else 9)).all() and got['counters'][1] == 0      # r = 1: the face neighbours at 0.01 m
        for i in range(len(pts)):
            near = np.array([kept[j][0] for j in got['rows'][i, :got['found'][i]].tolist()])
            assert np.abs(near - own[i]).max() <= r, (r, i)
        assert np.array_equal(np.array([kept[j][0] for j in got['rows'][:len(last), 0]]), own[:len(last)])     # a voxel centre finds its own voxel first
        mine = _host(host_exe, tmp_path, 'self_bound_r%d' % r)
        for i in range(mine['kept']):
            near = np.array([kept[j][0] for j in mine['rows'][i, :mine['found'][i]].tolist()]).reshape(-1, 3)
            assert np.abs(near - np.array(kept[i][0])).max(initial=0) <= r, (r, i)


BRUTE = [('dense11', 4, 16, 3.9), ('dense11', 2, 5, 1.9), ('dense11', 1, 2, 0.9), ('uniform', 2, 8, 1.9), ('uniform', 4, 16, 3.0), ('corner', 2, 8, 1.5)]


@pytest.mark.parametrize('scene,radius,k,voxels', BRUTE)
def test_the_result_is_the_global_k_nearest(scene, radius, k, voxels):
    """The theorem of the contract: for max_distance <= (r - 0.1) voxel_size the block search returns the k nearest kept centroids of the WHOLE map."""
    r = _scene(scene)
    rs = np.random.RandomState(int(10 * voxels) + k)
    base = {'dense11': _block_points(60, k, -0.62, 0.72), 'uniform': rs.uniform(-0.7, 0.7, (60, 3)).astype(np.float32),
            'corner': ah.corner(13, 20).astype(np.float32)}[scene]
    pts = np.concatenate([base, [[np.inf, 0, 0]]]).astype(np.float32)
    f = dict(min_count=2) if scene == 'corner' else dict()
    got = kref.knn(r, pts, k, radius=radius, max_distance=voxels * 0.1, **f)
    world, valid = kref.world_points(pts, r.voxel_size)
    rows, dist = kref.brute_force(r, k, world, voxels * 0.1, **f)
    assert np.array_equal(valid, got['status'] != I) and valid.sum() == len(pts) - 1
    assert np.array_equal(rows, got['rows'][valid]) and np.array_equal(ah.bits(dist), ah.bits(got['distance'][valid]))
    assert (got['found'] > 0).sum() > 10
    if scene != 'corner':                                                            # the self mode on the same map: 2^-16 of slack instead of 2^-17
        own = kref.neighbors(r, k, radius=radius, max_distance=voxels * 0.1)
        rows, dist = kref.brute_force(r, k, None, voxels * 0.1, self_mode=True)
        assert np.array_equal(rows, own['rows']) and np.array_equal(ah.bits(dist), ah.bits(own['distance']))


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_knn_workspace_bytes', 'pcacc_accum_knn', 'pcacc_accum_knn_self'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C16. ' in header and len(native._PROTOTYPES['pcacc_accum_knn']) == 22 and len(native._PROTOTYPES['pcacc_accum_knn_self']) == 21
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = open(os.path.join(csrc, 'accum_knn.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_register.h"']
    for helper in ('accr_world(', 'accr_candidate(', 'accn_column(', 'accn_centroid(', 'accum_unkey(', 'accum_field(', 'accn_index(', 'acck_next_column(', 'PCACC_BOUND(', 'PCACC_NO_CONTRACT'):
        assert helper in text, helper
    kernels = open(os.path.join(csrc, 'accum_knn.hip')).read()
    assert 'accn_rows_launch(' in kernels and 'accum_wave_count(' in kernels and 'asm' not in kernels and 'atomicAdd' not in kernels
    assert 'accum_knn.hip' in open(os.path.join(csrc, 'Makefile')).read()
    assert (native.KNN_MAX_K, native.KNN_MAX_RADIUS, native.KNN_INVALID, native.KNN_FOUND, native.KNN_FULL, native.KNN_COUNTERS) == (16, 4, 1, 2, 4, 5)
    assert (kref.MAX_K, kref.MAX_RADIUS, kref.INVALID, kref.FOUND, kref.FULL) == (16, 4, 1, 2, 4)
    for name, value in (('MAX_K', 16), ('MAX_RADIUS', 4), ('INVALID', 1), ('FOUND', 2), ('FULL', 4), ('COUNTERS', 5), ('N_QUERIES', 0), ('N_NEIGHBORS', 4)):
        assert ('#define PCACC_KNN_%s %d\n' % (name, value)) in header and getattr(native, 'KNN_' + name) == value
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.knn(torch.zeros(4, 3), 3)
    with pytest.raises(native.NativeError):
        cpu.neighbors(3)
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).knn(np.zeros((4, 3), np.float32), 3)
    for bad in (dict(k=0), dict(k=17), dict(k=3, radius=0), dict(k=3, radius=5), dict(k=3, max_distance=0.0), dict(k=3, max_distance=0.2000001),
                dict(k=3, radius=1, max_distance=0.11), dict(k=3, max_distance=float('nan'))):
        with pytest.raises(ValueError):                                              # before anything is allocated: a CPU map gets this far
            cpu.neighbors(**bad)
    with pytest.raises(ValueError):
        cpu.outliers(std_ratio=float('nan'))


def test_the_recorded_resource_usage_has_no_scratch():
    """profiles/accum_knn_resource_usage.txt (compile time): the running top-k stays in registers for every K, in both modes."""
    lines = [l for l in open(os.path.join(ROOT, 'profiles', 'accum_knn_resource_usage.txt')).read().split('\n') if l.startswith('  acck_')]     # the table's rows
    assert sorted(l.split()[0] for l in lines) == sorted('acck_%s_kernel<%d>' % (mode, K) for mode in ('point', 'self') for K in (1, 2, 4, 8, 16))
    assert all(' scratch 0 bytes/lane ' in l and ' VGPRs ' in l and ' waves/SIMD' in l for l in lines)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
_clouds = {}


def _cloud(scene):
    """A device map per scene, shared: the searches do not modify it (a test below says so)."""
    if scene not in _clouds:
        _clouds[scene] = ah.device_cloud(_scene(scene))
    return _clouds[scene]


def _poisoned(fields, rows):
    """Every byte of every output column 0xa5 (accum_host.h's POISON_BYTE), whatever its type."""
    return {name: torch.full((rows * int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size(),), 0xa5, dtype=torch.uint8, device=DEV)
            .view(dtype).reshape((rows,) + shape) for name, dtype, shape in fields}


def _search(m, points, args):
    """One call of the binding with every output and the counters poisoned first.  -> numpy columns as the host build's, and the device result."""
    from pcaccumulation_amd import native
    a = dict(args)
    k, radius, max_distance = m._knn_args(a.pop('k'), a.pop('radius'), a.pop('max_distance', None))
    counters = torch.full((5,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    f = (a.get('min_count', 1), a.get('max_moving_fraction'))
    m._ensure()
    if points is None:
        out = _poisoned(native.knn_fields(k, True), m.num_voxels)
        res = native.accum_knn_self(m.voxel_size, max_distance, k, radius, m._cur, m.num_voxels, *f, out=out, counters=counters)
        kept = int(res.pop('kept'))
        for name in kref.SELF_FIELDS:                                                # the rows behind the kept ones keep their poison
            assert bool((res[name][kept:].contiguous().view(torch.uint8) == 0xa5).all()), name
        res = {name: (t if name == 'counters' else t[:kept]) for name, t in res.items()}
    else:
        pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(DEV)
        out = _poisoned(native.knn_fields(k), pts.shape[0])
        res = native.accum_knn(pts, m._pose(a.get('pose')), m.voxel_size, max_distance, k, radius, m._cur, m.num_voxels, *f, out=out, counters=counters)
    return res


def _numpy(res):
    return {name: (t.tolist() if name == 'counters' else t.cpu().numpy()) for name, t in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernels_equal_the_host_build_gpu(host_exe, tmp_path, name):
    scene, points, args = CASES[name]
    host = _host(host_exe, tmp_path, name)
    m = _cloud(scene)
    snap = ah.snapshot(m, whole_sidecar=True)
    res = _search(m, points, args)
    assert all(t.is_cuda for t in res.values()) and res['counters'].dtype == torch.int64
    _assert_same(_numpy(res), host, name)
    again = _search(m, points, args)                                                 # a second run gives the same bits
    assert all(torch.equal(res[f].view(torch.int64) if res[f].dtype == torch.float64 else res[f],
                           again[f].view(torch.int64) if again[f].dtype == torch.float64 else again[f]) for f in res)
    method = m.neighbors(**args) if points is None else m.knn(torch.from_numpy(points).to(DEV), **args)     # the methods: the same call
    _assert_same(_numpy(method), host, name + ' (method)')
    ah.assert_unchanged(m, snap, name)                                                 # read-only: keys, records, stamps, state words, num_voxels


@pytest.mark.gpu
@pytest.mark.parametrize('scene', ['corner', 'uniform', 'tie'])
def test_k1_r1_is_query_gpu(scene):
    """knn(k=1, radius=1, max_distance=d) gives the row and distance bits of query(max_distance=d): the arithmetic and the tie rule are the same."""
    m = _cloud(scene)
    rs = np.random.RandomState(17)
    pts = {'corner': ah.corner(12, 300).astype(np.float32), 'uniform': rs.uniform(-0.7, 0.7, (900, 3)).astype(np.float32),
           'tie': np.concatenate([TIE_POINTS, rs.uniform(-0.1, 0.6, (200, 3)).astype(np.float32)])}[scene]
    pts = torch.from_numpy(pts).to(DEV)
    for frac, f in ((1.0, dict()), (0.5, dict()), (0.9, dict() if scene == 'tie' else dict(min_count=2))):     # every record of the tie scene has one point
        d = frac * m.voxel_size
        q, n = m.query(pts, max_distance=d, **f), m.knn(pts, 1, radius=1, max_distance=d, **f)
        assert torch.equal(q['row'], n['rows'][:, 0]) and torch.equal(q['distance'].view(torch.int64), n['distance'][:, 0].view(torch.int64)), (scene, frac)
        assert torch.equal((q['status'] & qref.MATCHED) != 0, n['found'] == 1) and int(n['counters'][2]) == int(q['counters'][4])
        assert int(n['counters'][2]) > 0


@pytest.mark.gpu
def test_self_mode_is_symmetric_gpu():
    """Where neither list is full, j is in i's list iff i is in j's, with equal distance bits."""
    m = _cloud('rows343')
    got = m.neighbors(16, radius=1)
    rows, dist, found = got['rows'].cpu().numpy(), got['distance'].cpu().numpy(), got['found'].cpu().numpy()
    open_ = found < 16
    assert 50 < open_.sum() and rows.shape == (343, 16)
    pairs = {(i, int(j)): ah.bits(dist[i, s:s + 1])[0] for i in np.flatnonzero(open_) for s, j in enumerate(rows[i, :found[i]]) if open_[j]}
    assert len(pairs) > 200 and all(pairs.get((j, i)) == b for (i, j), b in pairs.items())


@pytest.mark.gpu
@pytest.mark.parametrize('f', [dict(), FILTER], ids=['all', 'filtered'])
def test_neighbors_align_with_extract_gpu(f):
    m = _cloud('dense11' if not f else 'rows343')
    e, got = m.extract(**f), m.neighbors(8, radius=2, **f)
    v = e['points'].shape[0]
    assert got['rows'].shape == (v, 8) and got['mean_distance'].shape == (v,) and int(got['counters'][0]) == v > 0
    # the float64 centroids of extract's rows, from the records: count and coordinate sums in key order under the same filter
    keys, acc, _ = _scene('dense11' if not f else 'rows343').records()
    acc = acc.reshape(5, -1)
    keep = np.array([rref.keep(int(c), int(mv), f.get('min_count', 1), f.get('max_moving_fraction')) for c, mv in zip(acc[0], acc[1])])
    cen = (acc[2:5, keep].astype(np.float64) / acc[0, keep].astype(np.float64)) * (1.0 / 65536.0)
    assert np.array_equal(cen.T.astype(np.float32), e['points'].cpu().numpy())
    rows, dist, found = got['rows'].cpu().numpy(), got['distance'].cpu().numpy(), got['found'].cpu().numpy()
    have = np.arange(8)[None, :] < found[:, None]
    d = cen[:, :, None] - cen[:, np.where(have, rows, 0)]                              # [3, V, 8]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert np.array_equal(ah.bits(np.sqrt(d2)[have]), ah.bits(dist[have])) and (rows[have] < v).all() and (rows[~have] == -1).all()


def _assert_equals_restatement(m, r, pts, what, **args):
    got = m.knn(torch.from_numpy(pts).to(DEV), **args)
    _assert_same(_numpy(got), kref.knn(r, pts, **args), what)
    f = {a: args[a] for a in ('min_count', 'max_moving_fraction') if a in args}
    own = m.neighbors(**{a: v for a, v in args.items() if a != 'pose'})
    _assert_same(_numpy(own), kref.neighbors(r, **{a: v for a, v in args.items() if a != 'pose'}), what + ' (self)')
    assert own['found'].shape[0] == m.extract(**f)['points'].shape[0]                 # `rows` refers to the rows of the extract of that moment
    return got


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1)
    slab = ah.centres([(x, y, z) for x in (5, 6, 7) for y in range(-2, 3) for z in (-1, 0, 1)], 0.1)
    probe = np.concatenate([slab + np.float32(0.03), ah.centres([(9, 0, 0), (6, 9, 9), (-9, 0, 0)], 0.1), [[np.nan, 0, 0]]]).astype(np.float32)

    def both_add(pts, stamp):
        m.add(torch.from_numpy(pts).to(DEV), None, stamp=stamp)
        r.add(pts, None, stamp=stamp)
    both_add(np.concatenate([slab, slab[::2]]), 0)
    a = _assert_equals_restatement(m, r, probe, 'after add', k=5, radius=2, min_count=2)
    both_add(np.concatenate([slab[::3], ah.centres([(9, 1, 0), (6, 8, 9)], 0.1)]), 3)
    assert m.prune(before_stamp=2)['kept'] == rref.prune(r, None, before_stamp=2)[0] > 0      # what stamp 3 did not touch goes
    b = _assert_equals_restatement(m, r, probe, 'after prune', k=5, radius=2)
    assert int(b['counters'][4]) != int(a['counters'][4])
    both_add(ah.centres([(-9, 0, 0), (6, 0, 0), (6, 0, 0), (6, 9, 9)], 0.1), 4)
    c = _assert_equals_restatement(m, r, probe, 'add after prune', k=16, radius=4, pose=ah.rot_xyz(0, 0, 0.01, (0.01, 0.0, -0.01)))
    path = os.path.join(str(tmp_path), 'map.npz')
    m.save(path)
    d = _assert_equals_restatement(AccumulatedCloud.load(path, DEV), r, probe, 'after load', k=16, radius=4, pose=ah.rot_xyz(0, 0, 0.01, (0.01, 0.0, -0.01)))
    assert all(torch.equal(c[f], d[f]) for f in ('rows', 'found', 'status', 'counters'))


def test_the_outlier_scene_is_decided_by_the_restatement():
    """CPU: the restatement alone marks exactly the five floaters of the outlier scene."""
    r = _scene('outlier')
    kept = [c for c, _ in qref.kept_voxels(r)]
    mean, threshold, mask = kref.outliers(r, **OUTLIER_ARGS)
    assert len(kept) == 24 * 24 + 5 and int(mask.sum()) == 5 and sorted(kept[j] for j in np.flatnonzero(mask)) == sorted(FLOATERS)
    assert np.isposinf(mean).sum() == 1 and np.isfinite(threshold)                   # one floater sees nothing within 4 voxels, four see the sheet from afar
    sheet = np.array([c[2] == 0 for c in kept])
    assert mean[sheet].max() < 0.14 < threshold < 0.16 < mean[~sheet].min()


@pytest.mark.gpu
def test_outliers_remove_the_floaters_gpu():
    r = _scene('outlier')
    m = ah.device_cloud(r)
    mean, threshold, mask = kref.outliers(r, **OUTLIER_ARGS)
    got = m.outliers(**OUTLIER_ARGS)
    assert np.array_equal(ah.bits(got['mean_distance'].cpu().numpy()), ah.bits(mean))
    print('threshold: device %.17g, numpy %.17g' % (got['threshold'], threshold))
    assert abs(got['threshold'] - threshold) <= 1e-9 * threshold
    assert got['mask'].dtype == torch.bool and np.array_equal(got['mask'].cpu().numpy(), mask) and int(got['mask'].sum()) == 5
    e = m.extract()
    assert sorted(tuple(c) for c in e['coords'][got['mask']].tolist()) == sorted(FLOATERS)
    plane = m.select(got['mask'], invert=True)
    assert plane.num_voxels == 24 * 24 and bool((plane.extract()['coords'][:, 2] == 0).all()) and m.num_voxels == 24 * 24 + 5
    assert torch.equal(plane.extract()['points'], e['points'][~got['mask']])
    again = plane.outliers(**OUTLIER_ARGS)                               # what is left holds no row without a neighbour
    assert bool(torch.isfinite(again['mean_distance']).all())


@pytest.mark.gpu
def test_knn_results_on_the_model_forward_gpu(golden):
    """knn_results on the model_tiny_test forward runs and its counters sum.  Nothing more is claimed."""
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
    pose = ah.rot_xyz(0, 0, 0.01, (0.02, -0.01, 0.0))
    m = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, stamp=0)
    res = m.knn_results(out, inp, pose=pose, k=4, radius=2)
    same = m.knn(out['rec_est'], 4, pose, radius=2)
    assert all(torch.equal(res[k], same[k]) for k in ('rows', 'found', 'status', 'counters'))
    s, found = res['status'], res['found']
    n = out['rec_est'].shape[0]
    assert res['counters'].tolist() == [n, int(((s & I) != 0).sum()), int((found > 0).sum()), int((found == 4).sum()), int(found.sum())]
    assert int(res['counters'][2]) > 0
    with pytest.raises(ValueError):
        m.knn_results(dict(out, _n_batches=2), inp, k=4)


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    m = ah.device_cloud(_scene('rows65'))
    snap = ah.snapshot(m, whole_sidecar=True)
    n, k = 10, 5
    pts = torch.from_numpy(_block_points(n, 1)).to(DEV)
    out = {name: torch.full((n,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in native.knn_fields(k)}
    own = {name: torch.full((65,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in native.knn_fields(k, True)}
    counters = torch.full((5,), 7, dtype=torch.int64, device=DEV)
    good = dict(points=pts, pose=None, voxel_size=0.1, max_distance=0.2, k=k, radius=2, tables=m._cur, m=65, min_count=1, max_moving_fraction=None,
                out=out, counters=counters)
    bads = (dict(m=-1), dict(m=m.capacity + 1), dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float('inf')), dict(voxel_size=float('nan')),
            dict(max_distance=0.0), dict(max_distance=-0.05), dict(max_distance=0.2000001), dict(max_distance=float('nan')), dict(radius=1),
            dict(radius=0, max_distance=0.05), dict(radius=5), dict(k=0, out={f: t[:, :0] if t.dim() == 2 else t for f, t in out.items()}),
            dict(k=17, out={f: t.repeat(1, 4)[:, :17].contiguous() if t.dim() == 2 else t for f, t in out.items()}))
    for bad in bads:
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_knn(**dict(good, **bad))
        if 'k' in bad or 'm' in bad:                                                 # self mode: its k and m are the sizes of `own`; the raw calls below
            continue
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_knn_self(**dict({a: v for a, v in good.items() if a not in ('points', 'pose')}, out=own, **bad))
    lib = native.lib()
    ptr = [native._dev(out[name]) for name, _, _ in native.knn_fields(k)]
    optr = [native._dev(own[name]) for name, _, _ in native.knn_fields(k, True)]
    keys, acc, _ = (native._dev(t) for t in m._cur)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    kept = torch.full((1,), 7, dtype=torch.int64, device=DEV)

    def call(n_points=n, points=native._dev(pts), ptr=ptr, keys=keys, acc=acc, cnt=native._dev(counters), ws=native._dev(ws), ws_bytes=ws.numel()):
        return lib.pcacc_accum_knn(points, n_points, None, 0.1, 0.2, k, 2, keys, acc, m.capacity, 65, 1, 0, 0.0, *ptr, cnt, ws, ws_bytes, native._stream())

    def call_self(ptr=optr, keys=keys, acc=acc, out_n=native._dev(kept), cnt=native._dev(counters), ws=native._dev(ws), ws_bytes=ws.numel(), rows=65, k=k):
        return lib.pcacc_accum_knn_self(0.1, 0.2, k, 2, keys, acc, m.capacity, rows, 1, 0, 0.0, *ptr, out_n, cnt, ws, ws_bytes, native._stream())
    assert call(n_points=-1) == call(n_points=(1 << 30) + 1) == call(points=None) == call(keys=None) == call(acc=None) == call(cnt=None) == -1
    assert call(ws=None) == call(ws_bytes=16) == -1
    assert call_self(rows=-1) == call_self(rows=m.capacity + 1) == call_self(k=0) == call_self(k=17) == -1
    assert call_self(keys=None) == call_self(acc=None) == call_self(out_n=None) == call_self(cnt=None) == call_self(ws=None) == call_self(ws_bytes=16) == -1
    for j in range(len(ptr)):
        assert call(ptr=ptr[:j] + [None] + ptr[j + 1:]) == -1, j                     # a NULL output of non-zero size
    for j in range(len(optr)):
        assert call_self(ptr=optr[:j] + [None] + optr[j + 1:]) == -1, j
    need = native.ctypes.c_size_t(0)
    assert lib.pcacc_accum_knn_workspace_bytes(-1, native.ctypes.byref(need)) == lib.pcacc_accum_knn_workspace_bytes(65, None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in list(out.values()) + list(own.values()) + [counters, kept])     # nothing was launched: the poison stands
    ah.assert_unchanged(m, snap, 'bad arguments')
    for bad in (dict(k=0), dict(k=17), dict(k=5, radius=0), dict(k=5, radius=5), dict(k=5, max_distance=0.0), dict(k=5, max_distance=0.2000001),
                dict(k=5, max_distance=float('nan')), dict(k=5, pose=np.eye(3))):
        with pytest.raises(ValueError):
            m.knn(pts, **bad)
        if 'pose' not in bad:
            with pytest.raises(ValueError):
                m.neighbors(**bad)
            with pytest.raises(ValueError):
                m.outliers(**bad)
    with pytest.raises(ValueError):
        m.knn(pts[:, :2], 5)
    with pytest.raises(native.NativeError):
        m.knn(pts.cpu(), 5)
    zero = native.accum_knn(**dict(good, points=pts[:0], out={f: t[:0] for f, t in out.items()}))        # n = 0: the zero counters and nothing else
    assert zero['counters'].tolist() == [0] * 5 and all(bool((t == 7).all()) for t in out.values())
    assert call() == 0 and counters.tolist()[0] == n and not bool((out['status'] == 7).any())
    assert call_self() == 0 and counters.tolist()[0] == 65 == int(kept) and not bool((own['status'] == 7).any())
    ah.assert_unchanged(m, snap, 'after all')
