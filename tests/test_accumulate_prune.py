"""Removing rows from the accumulated scene cloud (include/pcacc.h C8): AccumulatedCloud.prune.

Every result is an integer or a copied record, so every claim is an equality:
  CPU   the g++ build of csrc/accum_prune.h (tests/accum_prune_host_driver.cpp, every table index asserted, poison behind the rows in use) against the
        plain-Python restatement on a coordinate dict (tests/accumulate_prune_reference.py): counters, surviving keys, records, stamps, ray counts;
  GPU   the kernels against the g++ build on the same scenes, then identities that tie prune to extract / normals / register / pierced, a life
        cycle against the restatement, the ghost scene of section 9f and a sliding box."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_pierce_reference as pref
import accumulate_prune_reference as rref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE, I32_MAX, I32_MIN
from helpers import ROOT

WHOLE_GRID = ((-EDGE,) * 3, (EDGE - 1,) * 3)


# ---- scenes: a ReferenceMap and a {coord: rays} dict (None: no sidecar), built once and never modified ----------------------------------------
# (voxel, points, moving) of tests/test_accumulate.py's ratio test: 1 of 4 sits exactly on 0.25; 1 of 3 and 2 of 4 above; 0 of 2 and 0 of 1 below; 4 of 4
RATIO_SPEC = [((2, 0, 0), 4, 1), ((-1, 3, 0), 3, 1), ((0, 0, 5), 4, 2), ((0, -2, 1), 2, 0), ((-7, 0, 0), 1, 0), ((2, 0, -1), 4, 4), ((0, 0, -5), 8, 2)]
RATIO_FILTERS = ((dict(min_count=1), 7), (dict(min_count=4), 4), (dict(min_count=5), 1), (dict(min_count=9), 0), (dict(max_moving_fraction=0.25), 4),
                 (dict(max_moving_fraction=float(np.nextafter(0.25, 0))), 2), (dict(max_moving_fraction=0.0), 2),
                 (dict(min_count=3, max_moving_fraction=1.0 / 3.0), 3), (dict(min_count=4, max_moving_fraction=0.25), 2),
                 (dict(max_moving_fraction=1.0), 7))

# the reason order: every row satisfies the named tests and no earlier one -- (count, moving, t_first, t_last), rays; box x in [0, 9], before_stamp 5
ORDER_ROWS = {(0, 0, 0): ((1, 0, 0, 9), 0, 'kept'), (1, 0, 0): ((1, 1, 0, 2), 9, 'filter'),       # filter + stale + pierced
              (12, 0, 0): ((1, 1, 0, 2), 9, 'filter'),                                               # filter + stale + box + pierced
              (2, 0, 0): ((1, 0, 0, 4), 9, 'stale'), (13, 0, 0): ((1, 0, 0, 4), 9, 'stale'),         # stale + pierced; stale + box + pierced
              (14, 0, 0): ((1, 0, 0, 5), 9, 'box'), (15, 0, 0): ((1, 0, 0, 9), 0, 'box'),            # box + pierced; box alone
              (3, 0, 0): ((1, 0, 0, 5), 3, 'pierced'), (4, 0, 0): ((1, 0, 0, 5), 2, 'kept')}
ORDER_ARGS = dict(max_moving_fraction=0.5, before_stamp=5, box=((0, -1, -1), (9, 1, 1)), min_pierced=3)


ROW_COUNTS = (0, 1, 63, 64, 65, 257)
_scenes = {}


def _build_scene(name):
    if name == 'rows_no_sidecar':
        return ah.records(0.1, ah.random_rows(65, 7)[0]), None
    if name.startswith('rows'):
        rows, pierced = ah.random_rows(int(name[4:]), 100 + int(name[4:]))
        return ah.records(0.1, rows), pierced
    if name == 'ratio':
        return ah.records(1.0, {v: (k, j, 0, 0) for v, k, j in RATIO_SPEC}), None
    if name == 'order':
        return ah.records(0.1, {c: v[0] for c, v in ORDER_ROWS.items()}), {c: v[1] for c, v in ORDER_ROWS.items() if v[1]}
    if name == 'stamps':                                                         # t_last = 4, 5, 6 and the ends of int32
        return ah.records(0.1, {(k, 0, 0): (1, 0, t, t) for k, t in enumerate((4, 5, 6, I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX))}), None
    if name == 'rays':                                                           # (count, rays): p / count against 0.5 and 1/3, p against min_pierced 2
        spec = [(4, 2), (4, 3), (3, 1), (6, 2), (6, 3), (1000, 2), (2, 1), (2, 2), (1, 5)]
        return (ah.records(0.1, {(k, 2, -1): (c, 0, 0, 0) for k, (c, _) in enumerate(spec)}), {(k, 2, -1): p for k, (_, p) in enumerate(spec)})
    if name == 'block7':                                                         # the full 7^3 block: every face of a box
        return ah.records(0.1, {(x, y, z): (1, 0, 0, 0) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)}), None
    if name == 'bound':
        vox, decoys = ah.bound_voxels()
        return ah.points_map(0.01, [(ah.centres(vox + decoys, 0.01), None, 0)]), None
    if name == 'plane':
        return ah.points_map(0.1, [(ah.noisy_plane(), None, 0)]), None
    if name == 'block27':
        return ah.records(0.1, {(x, y, z): (1, 0, 0, 0) for x in range(3) for y in range(3) for z in range(3)}), None
    if name == 'row9':
        return ah.records(0.1, {(k, 4, -2): (1, 0, 0, 0) for k in range(-4, 5)}), None
    if name == 'single':
        return ah.records(0.1, {(4, -12, 0): (1, 0, 0, 0)}), None
    if name == 'saved':
        # X has one neighbour, Y, which stage A removes (count 1): X is isolated although Y "would have saved" it.  P Q R in a row: Q keeps its 3
        # neighbours of stage A although P and R leave in stage B.
        rows = {(0, 0, 0): (5, 0, 0, 0), (1, 0, 0): (1, 0, 0, 0), (10, 0, 0): (5, 0, 0, 0), (11, 0, 0): (5, 0, 0, 0), (12, 0, 0): (5, 0, 0, 0)}
        return ah.records(0.1, rows), None
    assert name == 'wavy'
    return ah.points_map(0.1, [(ah.wavy(), None, 0)]), None


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene and the arguments of one prune (box in voxel indices) ---------------------------------------------------------------------------
ALONE = {'filter': dict(min_count=2, max_moving_fraction=0.25), 'stale': dict(before_stamp=8), 'box': dict(box=((-2, -1, -3), (1, 2, 0))),
         'pierced': dict(min_pierced=2), 'ratio': dict(min_pierced=1, ratio=0.5), 'isolated': dict(min_neighbors=8, radius=1)}
TOGETHER = dict(min_count=2, max_moving_fraction=0.5, before_stamp=4, box=((-3, -2, -3), (2, 3, 3)), min_pierced=2, ratio=0.4, min_neighbors=5, radius=1)
STAGE_B = {1: 9, 2: 20, 3: 30}


def _cases():
    cases = {}
    for m in ROW_COUNTS:
        for tag, args in ALONE.items():
            cases['rows%d_%s' % (m, tag)] = ('rows%d' % m, args)
        cases['rows%d_together' % m] = ('rows%d' % m, TOGETHER)
    cases['no_sidecar_min_pierced'] = ('rows_no_sidecar', dict(min_pierced=1))
    cases['keeps_nothing'] = ('rows65', dict(min_count=10 ** 6))
    cases['keeps_everything'] = ('rows65', dict())
    cases['whole_grid_box'] = ('bound', dict(box=WHOLE_GRID))
    cases['order'] = ('order', ORDER_ARGS)
    for k, (f, _) in enumerate(RATIO_FILTERS):
        cases['ratio_filter%d' % k] = ('ratio', f)
    for s in (4, 5, 6, I32_MIN, I32_MIN + 1, I32_MAX):
        cases['stale_before_%d' % s] = ('stamps', dict(before_stamp=s))
    cases['rays_half'] = ('rays', dict(min_pierced=2, ratio=0.5))
    cases['rays_third'] = ('rays', dict(min_pierced=1, ratio=1.0 / 3.0))
    cases['rays_count'] = ('rays', dict(min_pierced=2))
    cases['rays_ratio_zero'] = ('rays', dict(min_pierced=1, ratio=0.0))
    cases['box_faces'] = ('block7', dict(box=((-1, 0, -2), (1, 2, 0))))
    cases['box_one_voxel'] = ('block7', dict(box=((2, 2, 2), (2, 2, 2))))
    for r, n in STAGE_B.items():
        for scene in ('plane', 'block27', 'row9', 'single', 'bound'):
            cases['%s_r%d' % (scene, r)] = (scene, dict(min_neighbors=n, radius=r))
    cases['block27_corners_r1'] = ('block27', dict(min_neighbors=9, radius=1))
    cases['single_survives'] = ('single', dict(min_neighbors=1, radius=3))
    cases['saved_neighbour'] = ('saved', dict(min_count=2, min_neighbors=2, radius=1))
    cases['saved_chain'] = ('saved', dict(min_count=2, min_neighbors=3, radius=1))
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)


def _copy(r, pierced):
    c = ref.ReferenceMap(r.voxel_size)
    c.rec = {k: list(v) for k, v in r.rec.items()}
    c.dropped = r.dropped
    return c, (None if pierced is None else dict(pierced))


_restated = {}


def _restate(name):
    """The restatement's result of a case, computed once: counters, surviving records and ray counts in key order, k per stage-A survivor."""
    if name not in _restated:
        scene, args = CASES[name]
        r, pierced = _copy(*_scene(scene))
        _, k = rref.reasons(r, pierced, **args)
        counters = rref.prune(r, pierced, **args)
        keys, acc, stamps = r.records()
        _restated[name] = dict(counters=counters, keys=keys, acc=acc.reshape(5, -1), stamps=stamps.reshape(2, -1),
                               pierced=None if pierced is None else ah.aligned(pierced, keys), k=k)
    return _restated[name]


# ---- the host build -------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_prune_host_driver', 'prune_host')


def _run_host(exe, tmp_path, tag, records, pierced, spare_in=3, spare_out=5, min_count=1, max_moving_fraction=None, before_stamp=None, box=None, min_pierced=0,
              ratio=None, min_neighbors=0, radius=1):
    m = records[0].shape[0]
    lo, hi = ((0, 0, 0), (0, 0, 0)) if box is None else box
    head = [m, m + spare_in, m + spare_out, 0 if pierced is None else 1, min_count, 0 if max_moving_fraction is None else 1,
            0 if before_stamp is None else 1, 0 if before_stamp is None else before_stamp, 0 if box is None else 1] + list(lo) + list(hi) + [
            min_pierced, 0 if ratio is None else 1, min_neighbors, radius]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64),
                        np.array([0.0 if max_moving_fraction is None else max_moving_fraction, 0.0 if ratio is None else ratio], np.float64),
                        ah.map_bytes(*records, pierced))
    counters = np.frombuffer(raw, np.int64, 6).tolist()
    out, off = ah.unpack(raw, 48, ah.map_layout(counters[0], pierced is not None) + [('k', np.int32, (m,)), ('reason', np.uint8, (m,))])
    assert off == len(raw)
    if pierced is None:
        out['pierced'] = None
    return dict(out, counters=counters)


_hosted = {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, args = CASES[name]
        r, pierced = _scene(scene)
        keys = r.records()[0]
        _hosted[name] = _run_host(exe, tmp_path, name, r.records(), None if pierced is None else ah.aligned(pierced, keys), **args)
    return _hosted[name]


def _assert_same(got, want, what, pierced=True):
    assert list(got['counters']) == list(want['counters']), what
    for f in ('keys', 'acc', 'stamps'):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    if pierced:
        assert (got['pierced'] is None) == (want['pierced'] is None), what
        assert got['pierced'] is None or np.array_equal(got['pierced'], want['pierced']), what


# ---- CPU: host build == restatement ---------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    assert [_scene('rows%d' % m)[0].num_voxels for m in ROW_COUNTS] == list(ROW_COUNTS)
    assert _scene('wavy')[0].num_voxels == 76661 and 76661 % 64 != 0
    vox, decoys = ah.bound_voxels()
    assert _scene('bound')[0].num_voxels == len(set(vox + decoys)) and len(decoys) >= 36
    plane = _scene('plane')[0]
    assert plane.num_voxels > 900


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want, got = _restate(name), _host(host_exe, tmp_path, name)
    _assert_same(got, want, name)
    assert sum(got['counters']) == _scene(CASES[name][0])[0].num_voxels
    keys = _scene(CASES[name][0])[0].records()[0]
    if CASES[name][1].get('min_neighbors', 0) > 0:                                # the neighbour counts, voxel by voxel
        k = {rref.coord_of(int(key)): int(v) for key, v in zip(keys.tolist(), got['k'].tolist()) if v >= 0}
        assert k == want['k'], name
    else:
        assert (got['k'] == -1).all()


def test_reason_order_and_the_counts_it_gives(host_exe, tmp_path):
    r, pierced = _scene('order')
    why, _ = rref.reasons(r, pierced, **ORDER_ARGS)
    assert {c: rref.NAMES[w] for c, w in why.items()} == {c: v[2] for c, v in ORDER_ROWS.items()}
    got = _host(host_exe, tmp_path, 'order')
    keys = r.records()[0]
    assert [rref.NAMES[w] for w in got['reason'].tolist()] == [ORDER_ROWS[rref.coord_of(int(k))][2] for k in keys.tolist()]
    assert got['counters'] == [2, 2, 2, 2, 1, 0]


def test_exact_boundaries(host_exe, tmp_path):
    kept = lambda name: {rref.coord_of(int(k))[0] for k in _host(host_exe, tmp_path, name)['keys'].tolist()}
    # stamps sit at x = 0..6: 4, 5, 6, min, min + 1, max - 1, max.  t_last == before_stamp stays, before_stamp - 1 goes.
    assert kept('stale_before_5') == {1, 2, 5, 6} and kept('stale_before_4') == {0, 1, 2, 5, 6} and kept('stale_before_6') == {2, 5, 6}
    assert kept('stale_before_%d' % I32_MIN) == set(range(7)) and kept('stale_before_%d' % (I32_MIN + 1)) == set(range(7)) - {3}
    assert kept('stale_before_%d' % I32_MAX) == {6}
    # (count, rays) at x = 0..8: (4, 2) (4, 3) (3, 1) (6, 2) (6, 3) (1000, 2) (2, 1) (2, 2) (1, 5)
    assert kept('rays_half') == {0, 2, 3, 4, 5, 6}                               # 2 / 4 and 3 / 6 sit on 0.5 and stay; (3, 1), (2, 1): p < min_pierced
    assert kept('rays_third') == {2, 3, 5}                                       # 1 / 3 and 2 / 6 sit on the double 1 / 3 and stay
    assert kept('rays_count') == {2, 6}                                          # p == min_pierced goes, min_pierced - 1 stays
    assert kept('rays_ratio_zero') == set()                                      # every p >= 1 has p / count > 0
    for k, (_, n) in enumerate(RATIO_FILTERS):
        assert _host(host_exe, tmp_path, 'ratio_filter%d' % k)['counters'][:2] == [n, 7 - n], k
    assert _host(host_exe, tmp_path, 'no_sidecar_min_pierced')['counters'] == [65, 0, 0, 0, 0, 0]
    assert _host(host_exe, tmp_path, 'keeps_nothing')['counters'] == [0, 65, 0, 0, 0, 0]
    assert _host(host_exe, tmp_path, 'keeps_everything')['counters'] == [65, 0, 0, 0, 0, 0]


def test_box_faces(host_exe, tmp_path):
    got = _host(host_exe, tmp_path, 'box_faces')                                 # x in [-1, 1], y in [0, 2], z in [-2, 0] of the 7^3 block
    kept = {rref.coord_of(int(k)) for k in got['keys'].tolist()}
    assert kept == {(x, y, z) for x in (-1, 0, 1) for y in (0, 1, 2) for z in (-2, -1, 0)} and got['counters'] == [27, 0, 0, 316, 0, 0]
    for axis, (lo, hi) in enumerate(((-1, 1), (0, 2), (-2, 0))):
        for v, inside in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
            c = [0, 1, -1]
            c[axis] = v
            assert (tuple(c) in kept) == inside, (axis, v)
    assert _host(host_exe, tmp_path, 'box_one_voxel')['counters'] == [1, 0, 0, 342, 0, 0]
    whole = _host(host_exe, tmp_path, 'whole_grid_box')
    assert whole['counters'][0] == _scene('bound')[0].num_voxels and whole['counters'][3] == 0


def test_box_from_metres():
    """floor(bound / voxel_size) in float64, the map's own division: a bound on a voxel face belongs to the voxel above it when the division says so."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m = AccumulatedCloud(0.25, 'cpu', 64)                                         # 0.25 is exact: faces at multiples of 0.25
    box = ((-0.75, 0.0, 0.25), (0.5, 0.25, 1.0))
    assert m._box_indices(box) == ([-3, 0, 1], [2, 1, 4]) and rref.box_indices(box, 0.25) == ([-3, 0, 1], [2, 1, 4])
    t = AccumulatedCloud(0.1, 'cpu', 64)                                          # 0.3 / 0.1 = 2.9999999999999996: the point 0.3 lies in voxel 2
    assert t._box_indices(((0.3, -0.3, 0.7), (0.6, 0.3, 0.8))) == rref.box_indices(((0.3, -0.3, 0.7), (0.6, 0.3, 0.8)), 0.1)
    assert t._box_indices(((0.3, -0.3, 0.7), (0.6, 0.3, 0.8)))[0][0] == 2 == int(np.floor(np.float64(0.3) / np.float64(0.1)))
    assert t._box_indices(((-1e30, -1e9, 0), (1e30, 1e9, 0))) == ([-EDGE, -EDGE, 0], [EDGE - 1, EDGE - 1, 0])        # clamped into the grid
    for bad in (((0, 0, 0), (1, float('nan'), 1)), ((0, 0, 0), (1, float('inf'), 1)), ((0, 2, 0), (1, 1, 1)), ((0, 0), (1, 1, 1)), 5):
        with pytest.raises(ValueError):
            t._box_indices(bad)


def test_stage_b_on_the_restatement():
    """The literal neighbour counts of the small scenes, and the decoys of the index-bound scene."""
    assert sorted(_restate('block27_r1')['k'].values()) == sorted([8] * 8 + [12] * 12 + [18] * 6 + [27])
    assert _restate('block27_corners_r1')['counters'] == [19, 0, 0, 0, 0, 8]
    assert set(_restate('block27_r2')['k'].values()) == {27} and set(_restate('row9_r3')['k'].values()) == {4, 5, 6, 7}
    assert sorted(_restate('row9_r1')['k'].values()) == [2, 2, 3, 3, 3, 3, 3, 3, 3]
    assert _restate('single_r1')['counters'] == [0, 0, 0, 0, 0, 1] and _restate('single_survives')['counters'] == [1, 0, 0, 0, 0, 0]
    plane = _restate('plane_r1')
    assert plane['counters'][5] >= 30 and plane['counters'][0] > 700                # the strays (and the rim) leave, the sheet stays
    # stage B counts stage-A survivors: X is isolated because Y left in stage A; Q stays with k = 3 although P and R leave in stage B
    assert _restate('saved_neighbour')['counters'] == [3, 1, 0, 0, 0, 1] and _restate('saved_neighbour')['k'][(0, 0, 0)] == 1
    chain = _restate('saved_chain')
    assert chain['counters'] == [1, 1, 0, 0, 0, 3] and chain['k'][(11, 0, 0)] == 3 and [rref.coord_of(int(k)) for k in chain['keys']] == [(11, 0, 0)]
    # index bound: no voxel of a 3 x 3 column at an edge counts a decoy, at any radius
    vox, decoys = ah.bound_voxels()
    for r in (1, 2, 3):
        k = _restate('bound_r%d' % r)['k']
        for c in vox:
            near = sum(1 for v in set(vox + decoys) if max(abs(a - b) for a, b in zip(c, v)) <= r)
            assert k[c] == near, (r, c)


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_prune_workspace_bytes', 'pcacc_accum_prune'):
        assert ('int %s(' % name) in header
        assert name in native.EXPORTS
    assert ' C8. ' in header and len(native._PROTOTYPES['pcacc_accum_prune']) == 34
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_prune.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_normals.h"']
    assert 'accum_keep(' in text and 'accn_column(' in text and 'accum_merge_dst' in text
    assert (native.PRUNE_COUNTERS, native.PRUNE_KEPT, native.PRUNE_ISOLATED) == (6, 0, 5)
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.prune()
    with pytest.raises(native.NativeError):
        cpu.prune(min_pierced=1, dry_run=True)
    for bad in (dict(min_neighbors=3, radius=0), dict(min_neighbors=3, radius=4), dict(min_neighbors=344), dict(min_neighbors=-1), dict(min_pierced=-1),
                dict(pierced_ratio=0.5), dict(min_pierced=1, pierced_ratio=-0.1), dict(min_pierced=1, pierced_ratio=float('nan')),
                dict(before_stamp=1 << 31), dict(max_moving_fraction=float('nan')), dict(box=((0, 0, 0), (1, -1, 1))),
                dict(box=((0, 0, 0), (float('inf'), 1, 1)))):
        with pytest.raises(ValueError):                                          # before any call: the device is never asked
            cpu.prune(**bad)
    cpu_tables = (torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(native.NativeError):
        native.accum_prune(cpu_tables, 0, None, 1, None, None, None, 0, None, 0, 1, True, None, None, torch.zeros(6, dtype=torch.int64), None)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
def _device_cloud(r, pierced):
    """The restatement's map and {coord: rays} dict as an AccumulatedCloud on the device."""
    return ah.device_cloud(r, None if pierced is None else ah.aligned(pierced, r.records()[0]), np.zeros(5, np.int64))


def _metres(box, vs):
    """A box in voxel indices as metres whose floor(bound / voxel_size) gives the indices back: the middle of the face voxels."""
    return None if box is None else tuple(tuple((v + 0.5) * vs for v in side) for side in box)


def _prune(m, args, dry_run=False):
    a = dict(args)
    return m.prune(min_pierced=a.get('min_pierced') or None, pierced_ratio=a.get('ratio'), before_stamp=a.get('before_stamp'),
                   min_count=a.get('min_count', 1), max_moving_fraction=a.get('max_moving_fraction'), box=_metres(a.get('box'), m.voxel_size),
                   min_neighbors=a.get('min_neighbors') or None, radius=a.get('radius', 1), dry_run=dry_run)


def _assert_device_equals_host(m, res, host, what):
    t = lambda a: torch.from_numpy(a).to(DEV)
    assert [res[f] for f in rref.NAMES] == host['counters'] and all(type(res[f]) is int for f in rref.NAMES), what
    n = host['counters'][0]
    assert m.num_voxels == n, what
    keys, acc, stamps = m._cur
    assert torch.equal(keys[:n], t(host['keys'])) and torch.equal(acc[:, :n], t(host['acc'])) and torch.equal(stamps[:, :n], t(host['stamps'])), what
    assert (m._pierced is None) == (host['pierced'] is None), what
    if host['pierced'] is not None:
        assert m._pierced.shape[0] == m.capacity and torch.equal(m._pierced[:n], t(host['pierced'])), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    from pcaccumulation_amd import native
    scene, args = CASES[name]
    host = _host(host_exe, tmp_path, name)
    m = _device_cloud(*_scene(scene))
    before, state = ah.snapshot(m), m._state.tolist()
    dry = _prune(m, args, dry_run=True)
    assert [dry[f] for f in rref.NAMES] == host['counters'], name
    ah.assert_unchanged(m, before, name)                                            # dry_run: records, sidecar, num_voxels and the state words stay
    res = _prune(m, args)
    _assert_device_equals_host(m, res, host, name)
    state[native.ACCUM_NUM_VOXELS] = host['counters'][0]
    assert m._state.tolist() == state, name                                      # the state word is set on the device, the others are left alone
    again = _device_cloud(*_scene(scene))                                         # a second run gives the same map
    assert _prune(again, args) == res
    ah.assert_unchanged(again, ah.snapshot(m), name)


@pytest.mark.gpu
@pytest.mark.parametrize('args', [dict(min_neighbors=6, radius=1), dict(min_neighbors=6, radius=1, before_stamp=1), dict(box=((-100, -90, -5), (99, 100, 5)))],
                         ids=['isolated_r1', 'all_stale', 'box'])
def test_kernel_on_76661_voxels_gpu(host_exe, tmp_path, args):
    r, _ = _scene('wavy')
    host = _run_host(host_exe, tmp_path, 'wavy', r.records(), None, **args)
    m = _device_cloud(r, None)
    assert m.num_voxels == 76661
    res = _prune(m, args)
    _assert_device_equals_host(m, res, host, 'wavy')
    if 'box' not in args and 'before_stamp' not in args:
        assert res['isolated'] >= 1 and res['kept'] > 70000                       # the far voxel leaves, the sheet stays


# ---- identities: prune against extract, normals, register and pierced --------------------------------------------------------------------------------------
FILTER = dict(min_count=2, max_moving_fraction=0.0)


TRUE_POSE = ah.rot_xyz(np.deg2rad(0.6), np.deg2rad(-0.5), np.deg2rad(0.7), (0.02, -0.015, 0.017))


def _corner_cloud():
    """The room corner with a region predicted moving, two stamps: the filter min_count=2, max_moving_fraction=0.0 removes part of it."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    pts = ah.corner(11, 9000).astype(np.float32)
    mv = (pts[:, 0] > ah.CORNER[0] + 1.6) & (np.random.RandomState(4).uniform(0, 1, pts.shape[0]) < 0.5)
    m = AccumulatedCloud(0.1, DEV, 64)
    m.add(torch.from_numpy(pts[:15000]).to(DEV), moving=torch.from_numpy(mv[:15000]).to(DEV), stamp=3)
    m.add(torch.from_numpy(pts[15000:]).to(DEV), moving=torch.from_numpy(mv[15000:]).to(DEV), stamp=1)
    return m


def _corner_scan():
    inv = np.linalg.inv(TRUE_POSE)
    return torch.from_numpy((ah.corner(12, 1300) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)).to(DEV)


def _equal_dicts(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_prune_then_read_equals_the_filtered_read_gpu(host_exe, tmp_path):
    m = _corner_cloud()
    total = m.num_voxels
    cloud, nrm = m.extract(**FILTER), m.normals(radius=1, min_neighbors=5, **FILTER)
    reg = m.register(_corner_scan(), max_iter=6, **FILTER)
    assert 0 < cloud['count'].shape[0] < total and int(reg['correspondences']) > 1000
    # stage B's k and the isolated counter against normals' neighbour count on the same filter
    for radius, least in ((1, 7), (2, 14)):
        neighbors = m.normals(radius=radius, min_neighbors=5, **FILTER)['neighbors']
        host = _run_host(host_exe, tmp_path, 'corner%d' % radius, m.records(), None, min_neighbors=least, radius=radius, **FILTER)
        assert torch.equal(torch.from_numpy(host['k'][host['k'] >= 0]).to(DEV), neighbors), radius
        dry = m.prune(min_neighbors=least, radius=radius, dry_run=True, **FILTER)
        assert dry['isolated'] == int((neighbors < least).sum()) == host['counters'][5] and dry['filter'] == total - neighbors.shape[0], radius
    res = m.prune(**FILTER)
    assert res == dict(kept=cloud['count'].shape[0], filter=total - cloud['count'].shape[0], stale=0, box=0, pierced=0, isolated=0)
    for f in (FILTER, dict()):                                                   # the rows that are left all pass the filter: with or without it
        assert _equal_dicts(m.extract(**f), cloud)
        assert _equal_dicts(m.normals(radius=1, min_neighbors=5, **f), nrm)
        assert _equal_dicts(m.register(_corner_scan(), max_iter=6, **f), reg)


# ---- the ghost scene of section 9f, rebuilt here --------------------------------------------------------------------------------------------------------------
_ghost = {}


def _ghost_restatement():
    """The map and ray counts after the six scans, computed once; callers copy."""
    if not _ghost:
        r = ref.ReferenceMap(0.1)
        pierced, counters = {}, [0] * 5
        for k, (wall, cluster, _) in enumerate(ah.ghost_scans()):
            pts = np.concatenate([wall, cluster])
            pref.pierce(pref.voxels_of(r), pts, ah.GHOST_SENSOR, voxel_size=0.1, stamp=k, pierced=pierced, counters=counters)
            r.add(pts, stamp=k)
        _ghost['r'] = (r, pierced)
    return _copy(*_ghost['r'])


def _ghost_cloud():
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m = AccumulatedCloud(0.1, DEV, 64)
    for k, (wall, cluster, _) in enumerate(ah.ghost_scans()):
        pts = torch.from_numpy(np.concatenate([wall, cluster])).to(DEV)
        m.see_through(pts, ah.GHOST_SENSOR, stamp=k)
        m.add(pts, stamp=k)
    return m


def _assert_equals_restatement(m, r, pierced, what):
    keys, acc, stamps = r.records()
    got = m.records()
    assert m.num_voxels == r.num_voxels, what
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], acc.reshape(5, -1)) and np.array_equal(got[2], stamps.reshape(2, -1)), what
    if pierced is not None:
        assert np.array_equal(m._pierced[:m.num_voxels].cpu().numpy(), ah.aligned(pierced, keys)), what


@pytest.mark.gpu
def test_ghost_trail_is_removed_from_the_map_gpu():
    r, pierced = _ghost_restatement()
    m = _ghost_cloud()
    _assert_equals_restatement(m, r, pierced, 'ghost before')
    before = m.extract()
    seen = m.pierced()
    res = m.prune(min_pierced=1)
    want = rref.prune(r, pierced, min_pierced=1)
    assert [res[f] for f in rref.NAMES] == want
    _assert_equals_restatement(m, r, pierced, 'ghost after')
    after = m.extract()
    keep = seen < 1                                                              # the identity: the rows of the earlier extract where pierced() < 1
    assert all(torch.equal(after[f], before[f][keep]) for f in before)
    assert int(m.pierced().sum()) == 0
    coords = after['coords'].cpu().numpy()
    assert (coords[:, 0] == 30).sum() == 800                                     # every wall voxel survives
    scans = ah.ghost_scans()
    early = {v for k in range(5) for v in scans[k][2]}
    left = {tuple(c) for c in coords.tolist()}
    assert len(early) == 135 and len(early - left) >= 100                        # section 9f's figures, now gone from the map itself
    nrm = m.normals(radius=1, min_neighbors=5)
    removed = {tuple(c) for c in before['coords'].cpu().tolist()} - left
    assert len(removed) == res['pierced'] and nrm['normals'].shape[0] == coords.shape[0] and not removed & left   # no normal at a removed voxel


# ---- life cycle against the restatement --------------------------------------------------------------------------------------------------------------------
def _both_add(m, r, idx, stamp):
    pts = ah.centres(idx, r.voxel_size)
    m.add(torch.from_numpy(pts).to(DEV), stamp=stamp)
    r.add(pts, stamp=stamp)


def _both_see(m, r, pierced, targets, stamp):
    pts = ah.centres(targets, r.voxel_size)
    m.see_through(torch.from_numpy(pts).to(DEV), np.array([[0.05, 0.05, 0.05]]), stamp=stamp)
    pref.pierce(pref.voxels_of(r), pts, np.array([[0.05, 0.05, 0.05]]), voxel_size=r.voxel_size, stamp=stamp, pierced=pierced)


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, pierced = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), {}
    slab = [(x, y, z) for x in (5, 6, 7) for y in range(-2, 3) for z in (-1, 0, 1)]
    _both_add(m, r, slab, 0)
    _both_see(m, r, pierced, [(20, y, 0) for y in (-2, 0, 3)], 1)                # rays along +x through the slab
    gone = [c for c in slab if pierced.get(c, 0) >= 1]
    assert (6, 0, 0) in gone and 3 <= len(gone) < len(slab)
    res = m.prune(min_pierced=1)
    assert [res[f] for f in rref.NAMES] == rref.prune(r, pierced, min_pierced=1) and res['pierced'] == len(gone)
    _assert_equals_restatement(m, r, pierced, 'first prune')
    assert m.capacity == 64 and m.dropped == 0
    # add after a prune: new voxels below, between and above the map's keys, one of them a voxel that was just removed
    cube = [(x, y, z) for x in (6, 7) for y in (9, 10) for z in (9, 10)]
    _both_add(m, r, [(-9, 0, 0), (6, 0, 0), (6, 0, 0), (30, 1, 1)] + cube, 2)
    _assert_equals_restatement(m, r, pierced, 'add after prune')
    back = r.rec[rref.key_of((6, 0, 0))]
    assert back[0] == 2 and back[5:] == [2, 2] and pierced.get((6, 0, 0), 0) == 0  # the new points only, fresh stamps, no rays
    row = int(np.searchsorted(m.records()[0], rref.key_of((6, 0, 0))))
    assert m.records()[1][0, row] == 2 and m.records()[2][:, row].tolist() == [2, 2] and int(m._pierced[row]) == 0
    _both_see(m, r, pierced, [(20, 2, 3), (20, -6, 0), (28, 1, 1)], 3)
    res = m.prune(min_pierced=1, before_stamp=1, min_neighbors=2, radius=1)
    assert [res[f] for f in rref.NAMES] == rref.prune(r, pierced, min_pierced=1, before_stamp=1, min_neighbors=2, radius=1)
    assert res['stale'] > 0 and res['isolated'] > 0 and res['kept'] >= 8       # the slab is stale, the single voxels are isolated, the cube stays
    _assert_equals_restatement(m, r, pierced, 'second prune')
    path = os.path.join(str(tmp_path), 'pruned.npz')
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['acc', 'dropped', 'keys', 'pierce_counters', 'pierced', 'stamps', 'voxel_size']
    loaded = AccumulatedCloud.load(path, DEV)
    assert m.capacity == 64 and m.num_voxels < 64
    big = [(x, y, z) for x in range(-8, 8) for y in range(-8, 8) for z in range(40, 56)]        # 4096 new voxels: 64 -> 8192 rows
    for cloud in (m, loaded):
        cloud.add(torch.from_numpy(ah.centres(big + [(6, 0, 0)], 0.1)).to(DEV), stamp=4)
        assert cloud.capacity >= 4096
        cloud.see_through(torch.from_numpy(ah.centres([(0, 0, 70)], 0.1)).to(DEV), np.array([[0.05, 0.05, 0.05]]), stamp=5)
    r.add(ah.centres(big + [(6, 0, 0)], 0.1), stamp=4)
    pref.pierce(pref.voxels_of(r), ah.centres([(0, 0, 70)], 0.1), np.array([[0.05, 0.05, 0.05]]), voxel_size=0.1, stamp=5, pierced=pierced)
    want = rref.prune(r, pierced, min_pierced=1, box=rref.box_indices(((-0.45, -0.8, 0.0), (0.75, 0.8, 9.0)), 0.1))
    for cloud in (m, loaded):
        res = cloud.prune(min_pierced=1, box=((-0.45, -0.8, 0.0), (0.75, 0.8, 9.0)))
        assert [res[f] for f in rref.NAMES] == want and res['pierced'] > 0 and res['box'] > 0
        _assert_equals_restatement(cloud, r, pierced, 'after growth')


@pytest.mark.gpu
def test_sliding_box_keeps_the_map_local_gpu():
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, unpruned = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), ref.ReferenceMap(0.1)
    rs = np.random.RandomState(33)
    for k in range(8):
        centre = np.array([0.45 * k, -0.2 * k, 0.05 * k])
        pts = (centre + rs.uniform(-1.0, 1.0, (300, 3))).astype(np.float32)
        m.add(torch.from_numpy(pts).to(DEV), stamp=k)
        r.add(pts, stamp=k)
        unpruned.add(pts, stamp=k)
        box = (tuple(centre - 1.0), tuple(centre + 1.0))
        res = m.prune(box=box)
        want = rref.prune(r, None, box=rref.box_indices(box, 0.1))
        assert [res[f] for f in rref.NAMES] == want and (k == 0 or res['box'] > 0), k
        assert m.num_voxels == r.num_voxels <= 21 ** 3, k
        _assert_equals_restatement(m, r, None, 'window %d' % k)
        assert k == 0 or m.num_voxels < unpruned.num_voxels, k                   # it no longer grows with the drive


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    r, pierced = _scene('rows65')
    m = _device_cloud(r, pierced)
    snap = ah.snapshot(m)
    out = tuple(torch.full_like(t, 7) for t in m._cur)
    pout = torch.full_like(m._pierced, 7)
    counters = torch.full((6,), 7, dtype=torch.int64, device=DEV)
    good = dict(tables_in=m._cur, m=65, pierced_in=m._pierced, min_count=1, max_moving_fraction=None, before_stamp=None, box=None, min_pierced=0, ratio=None,
                min_neighbors=0, radius=1, dry_run=False, tables_out=out, pierced_out=pout, counters=counters, state=m._state)
    small = tuple(t[..., :64].contiguous() for t in out)
    lo, hi = (0, 0, 0), (1, 1, 1)
    for bad in (dict(m=-1), dict(m=m.capacity + 1), dict(tables_out=small, pierced_out=pout[:64].contiguous()), dict(tables_out=m._cur),
                dict(pierced_out=m._pierced), dict(tables_out=(out[0], m._cur[1], out[2])), dict(min_neighbors=3, radius=0), dict(min_neighbors=3, radius=4),
                dict(min_neighbors=344), dict(min_neighbors=-1), dict(ratio=float('nan')), dict(ratio=-0.5), dict(box=((2, 0, 0), hi)),
                dict(box=(lo, (1, 1, EDGE))), dict(box=((-EDGE - 1, 0, 0), hi))):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_prune(**dict(good, **bad))
    torch.cuda.synchronize()
    ah.assert_unchanged(m, snap, 'bad arguments')
    assert all(bool((t == 7).all()) for t in out + (pout, counters))
    native.accum_prune(**dict(good, m=0))                                        # m = 0: the zero counters and nothing else
    assert counters.tolist() == [0] * 6 and all(bool((t == 7).all()) for t in out + (pout,))
    ah.assert_unchanged(m, snap, 'm = 0')
    for bad in (dict(radius=4, min_neighbors=2), dict(min_neighbors=344), dict(pierced_ratio=1.0), dict(box=((0, 0, 0), (float('nan'), 1, 1))),
                dict(box=((1, 0, 0), (0, 1, 1)))):
        with pytest.raises(ValueError):
            m.prune(**bad)
    ah.assert_unchanged(m, snap, 'ValueError')
    assert m.prune(dry_run=True) == dict(kept=65, filter=0, stale=0, box=0, pierced=0, isolated=0)
