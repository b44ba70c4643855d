"""Two accumulated scene clouds compared, and the rows of extract() that a mask names as a new map (include/pcacc.h C13):
AccumulatedCloud.compare, .select and .difference.

Every result is an integer, a copied record or a float64 computed in one order, so every claim is an equality (float64 as bits):
  CPU   the g++ build of csrc/accum_compare.h (tests/accum_compare_host_driver.cpp: every table index asserted, poison behind the rows in use, every
        output row written exactly once, a refused select leaves every output row poison) against the plain-numpy restatement
        (tests/accumulate_compare_reference.py);
  GPU   the kernels against the g++ build on the same scenes; compare against query() on maps whose float64 centroids are their points; the rows
        against extract() under a filter; the counters against merge's; select against copy() + prune(), against merge() of its two halves and against
        extract() indexed by the mask; difference against select() built by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import accumulate_compare_reference as cref
import accumulate_helpers as ah
import accumulate_merge_reference as mref
import accumulate_reference as ref
from accumulate_helpers import DEV
from helpers import ROOT

COLUMNS = (('status', np.uint8), ('same_row', np.int32), ('row', np.int32), ('distance', np.float64), ('pierced', np.int32))
SIDES = (('self', 'a'), ('other', 'b'))


# ---- scenes (those of tests/test_accumulate_merge.py): (ReferenceMap, {key: rays} or None), built once and never modified -------------------------------
ROW_COUNTS = (0, 1, 63, 64, 65)


def _dense(seed, rays_seed=None):
    """Many points per voxel, three stamps, flags, dropped points."""
    r = ref.ReferenceMap(0.1)
    for k in range(3):
        pts = np.random.RandomState(seed + k).uniform((-1, -1, -0.5), (1, 1, 0.5), (3000, 3)).astype(np.float32)
        pts[::501] = np.nan
        r.add(pts, None, np.random.RandomState(seed + 10 + k).uniform(0, 1, 3000) < 0.3, stamp=5 - 2 * k)
    if rays_seed is None:
        return r, None
    rs = np.random.RandomState(rays_seed)
    return r, {k: int(rs.randint(0, 9)) for k in r.rec}


def _exact_points(seed, n):
    """Points on the 2^-10 m grid of a 2 m x 2 m x 1 m box, at most one per 0.1 m voxel: exact in float32 and in 2^-16 fixed point."""
    rs = np.random.RandomState(seed)
    grid = rs.randint((-1024, -1024, -512), (1024, 1024, 512), (n, 3))
    pts = (grid.astype(np.float64) * 2.0 ** -10).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) * 1024.0, grid.astype(np.float64))
    _, key, _ = ref.per_point(pts, None, 0.1)
    return pts[np.unique(key, return_index=True)[1]]


_scenes = {}


def _build_scene(name):
    if name.startswith('rows'):                                                  # rows<m>_<seed>: with a sidecar
        m, seed = (int(v) for v in name[4:].split('_'))
        return ah.rows(ah.some(m, seed), 50 + 7 * m + seed, rays=True)
    line = lambda xs: [(x, 1, -1) for x in xs]
    if name == 'low':
        return ah.rows(line(range(-40, -10)), 1)
    if name == 'high':
        return ah.rows(line(range(10, 47)), 2)
    if name == 'even':
        return ah.rows(line(range(-20, 20, 2)), 3)
    if name == 'odd':
        return ah.rows(line(range(-19, 21, 2)), 4)
    if name == 'outer':
        return ah.rows(line(range(-30, 30)), 5)
    if name == 'inner':
        return ah.rows(line(range(-7, 9)), 6)
    if name in ('plain_a', 'plain_b'):                                           # overlapping, no sidecar
        return ah.rows(ah.some(70, 11 if name == 'plain_a' else 12), 13 if name == 'plain_a' else 14)
    if name in ('rays_a', 'rays_b'):
        return ah.rows(ah.some(70, 11 if name == 'rays_a' else 12), 15 if name == 'rays_a' else 16, rays=True)
    if name in ('wavy', 'wavy_near', 'wavy_half'):
        r = ref.ReferenceMap(0.1)
        r.add(ah.wavy({'wavy': 0.0, 'wavy_near': 0.03, 'wavy_half': 13.0}[name]), stamp=3 if name == 'wavy' else 8)
        return r, None
    if name == 'dense':
        return _dense(30)
    if name == 'dense_b':
        return _dense(60, rays_seed=44)
    if name == 'exact_a':                                                        # one point per voxel, none moving
        return ref.ReferenceMap(0.1).add(_exact_points(90, 1500), stamp=2), None
    assert name == 'exact_b'                                                     # half of exact_a's points moved by up to 0.06 m, and others; some moving; rays
    pts = _scene('exact_a')[0].extract()['points']
    rs = np.random.RandomState(91)
    moved = pts[::2] + (rs.randint(-60, 61, (pts[::2].shape[0], 3)).astype(np.float64) * 2.0 ** -10).astype(np.float32)
    pts = np.concatenate([moved, _exact_points(92, 700)])
    r = ref.ReferenceMap(0.1).add(pts, None, rs.uniform(0, 1, pts.shape[0]) < 0.3, stamp=6)
    return r, {k: int(rs.randint(0, 7)) for k in r.rec}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: (scene A, scene B or None = A itself, max_distance, min_count, max_moving_fraction) ---------------------------------------------------------
COMPARE_CASES = {'below': ('high', 'low', 0.1, 1, None), 'above': ('low', 'high', 0.1, 1, None), 'interleaved': ('even', 'odd', 0.1, 1, None),
                 'contained': ('outer', 'inner', 0.1, 1, None), 'contains': ('inner', 'outer', 0.07, 1, None), 'identical': ('even', 'even', 0.1, 1, None),
                 'self': ('rows65_1', None, 0.1, 1, None), 'no_sidecar': ('plain_a', 'plain_b', 0.1, 1, None), 'sidecar_a': ('rays_a', 'plain_b', 0.08, 1, None),
                 'sidecar_b': ('plain_a', 'rays_b', 0.1, 2, None), 'sidecar_both': ('rays_a', 'rays_b', 0.05, 1, 0.5),
                 'filter': ('dense', 'dense_b', 0.1, 2, 0.5), 'exact': ('exact_a', 'exact_b', 0.05, 1, 0.0)}
for _ma in ROW_COUNTS:
    for _mb in ROW_COUNTS:
        COMPARE_CASES['rows_%d_%d' % (_ma, _mb)] = ('rows%d_1' % _ma, 'rows%d_2' % _mb, 0.1, 1, None)
SHEET_CASES = {'sheet_near': ('wavy', 'wavy_near', 0.1, 1, None), 'sheet_half': ('wavy', 'wavy_half', 0.1, 1, None)}
COMPARE_CASES.update(SHEET_CASES)
COMPARE_NAMES = sorted(COMPARE_CASES)

# (scene, mask rule, invert, min_count, max_moving_fraction); the mask has one entry per row the filter keeps unless the rule says otherwise
SELECT_CASES = {'rows%d' % m: ('rows%d_1' % m, 'random', False, 1, None) for m in ROW_COUNTS}
SELECT_CASES.update({'rows65_inverted': ('rows65_1', 'random', True, 1, None), 'rows65_filter': ('rows65_1', 'random', False, 3, 0.5),
                     'no_sidecar': ('plain_a', 'random', False, 2, None), 'all': ('rays_a', 'ones', False, 1, None), 'none': ('rays_a', 'ones', True, 1, None),
                     'dense': ('dense_b', 'random', False, 2, 0.5), 'sheet': ('wavy', 'third', False, 1, None), 'short': ('rows65_1', 'short', False, 1, None),
                     'long': ('rows64_1', 'long', True, 1, None), 'empty_long': ('rows0_1', 'long', False, 1, None)})
SELECT_NAMES = sorted(SELECT_CASES)


def _mask(name):
    scene, rule, _, min_count, mmf = SELECT_CASES[name]
    kept = _scene(scene)[0].extract(min_count, mmf)['count'].shape[0]
    if rule == 'ones':
        return np.ones(kept, np.uint8)
    if rule == 'third':
        return (np.arange(kept) % 3 == 0).astype(np.uint8)
    n = {'random': kept, 'short': kept - 1, 'long': kept + 1}[rule]
    return (np.random.RandomState(len(name) + kept).uniform(0, 1, n) < 0.5).astype(np.uint8) * 3      # non-zero, not only 1


# ---- the host build ----------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_compare_host_driver', 'compare_host')


def _map_bytes(r, pierced):
    keys, acc, stamps = r.records()
    return ah.map_bytes(keys, acc, stamps, None if pierced is None else mref.aligned(pierced, keys))


def _run_host_compare(exe, tmp_path, tag, a, b, max_distance, min_count, mmf, spare=3):
    """a, b = (ReferenceMap, rays); b None: B is A.  -> {'self': columns, 'other': columns, 'counters': [12]}."""
    (ra, pa), (rb, pb) = a, (a if b is None else b)
    head = [0, ra.num_voxels, ra.num_voxels + spare, 0 if pa is None else 1, rb.num_voxels, rb.num_voxels + spare, 0 if pb is None else 1,
            1 if b is None else 0, min_count, 0 if mmf is None else 1]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array([0.0 if mmf is None else mmf, max_distance], np.float64),
                        _map_bytes(ra, pa), b'' if b is None else _map_bytes(rb, pb))
    counters = np.frombuffer(raw, np.int64, 12).tolist()
    out, off = {'counters': counters}, 96
    for side, at in (('self', 0), ('other', 6)):
        out[side], off = ah.unpack(raw, off, [(name, dtype, (counters[at + 1],)) for name, dtype in COLUMNS])
    assert off == len(raw)
    return out


def _run_host_select(exe, tmp_path, tag, a, mask, invert, min_count, mmf, spare_in=3, spare_out=5):
    r, p = a
    m = r.num_voxels
    head = [1, m, m + spare_in, 0 if p is None else 1, m + spare_out, min_count, 0 if mmf is None else 1, mask.shape[0], 1 if invert else 0]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array([0.0 if mmf is None else mmf], np.float64), _map_bytes(r, p),
                        np.ascontiguousarray(mask, np.uint8))
    counters, state = np.frombuffer(raw, np.int64, 4).tolist(), np.frombuffer(raw, np.int64, 8, 32).tolist()
    out, off = ah.unpack(raw, 96, ah.map_layout(counters[3], p is not None))
    assert off == len(raw)
    if p is None:
        out['pierced'] = None
    return dict(out, counters=counters, state=state)


_hosted = {}


def _host_compare(exe, tmp_path, name):
    if ('c', name) not in _hosted:
        a, b, dist, min_count, mmf = COMPARE_CASES[name]
        _hosted[('c', name)] = _run_host_compare(exe, tmp_path, name, _scene(a), None if b is None else _scene(b), dist, min_count, mmf)
    return _hosted[('c', name)]


def _host_select(exe, tmp_path, name):
    if ('s', name) not in _hosted:
        scene, _, invert, min_count, mmf = SELECT_CASES[name]
        _hosted[('s', name)] = _run_host_select(exe, tmp_path, name, _scene(scene), _mask(name), invert, min_count, mmf)
    return _hosted[('s', name)]


_restated = {}


def _restatement(name):
    if name not in _restated:
        a, b, dist, min_count, mmf = COMPARE_CASES[name]
        (ra, pa), (rb, pb) = _scene(a), _scene(a if b is None else b)
        _restated[name] = cref.compare(ra, pa, rb, pb, dist, min_count, mmf)
    return _restated[name]


def _flat(counters):
    return [counters[side][k] for side in ('self', 'other') for k in cref.SIDE]


def _assert_columns(got, want, what):
    for name, dtype in COLUMNS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype == dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)     # float64 as bits


# ---- CPU: host build == restatement ----------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    for m in ROW_COUNTS:
        assert _scene('rows%d_1' % m)[0].num_voxels == m == _scene('rows%d_2' % m)[0].num_voxels
    shared = lambda a, b: len(set(_scene(a)[0].rec) & set(_scene(b)[0].rec))
    assert shared('rows65_1', 'rows65_2') not in (0, 65) and shared('even', 'odd') == 0 and shared('outer', 'inner') == 16 == _scene('inner')[0].num_voxels
    assert max(_scene('low')[0].rec) < min(_scene('high')[0].rec)
    assert _scene('wavy')[0].num_voxels == 76661 and 76661 % 64 != 0 and 76661 > 2048
    near, half = _restatement('sheet_near')['counters'], _restatement('sheet_half')['counters']
    assert near['self']['only'] < 1000 and near['self']['near'] > 75000 and 0 < near['self']['same'] < 76661      # mostly SAME / NEAR
    # half overlap: the sheet's half at x < 0 has nothing of the other above or below it, the other half meets it where the two surfaces cross
    assert 76661 // 2 - 300 < half['self']['only'] < 76661 and 1000 < half['self']['same'] < half['self']['held'] + 1 and half['self']['near'] > 1000
    f = _restatement('filter')                                                   # the filter removes rows on both sides; HELD without SAME occurs
    for side, scene in (('self', 'dense'), ('other', 'dense_b')):
        c = f['counters'][side]
        assert 0 < c['kept'] < c['rows'] == _scene(scene)[0].num_voxels and c['held'] > c['same'] > 0
        assert int(((f[side]['status'] & (cref.HELD | cref.SAME)) == cref.HELD).sum()) == c['held'] - c['same']
    e = _restatement('exact')['self']['status']                                  # matched, unmatched, held-but-filtered and absent voxels
    for bits, value in ((cref.NEAR, cref.NEAR), (cref.NEAR, 0), (cref.HELD | cref.SAME, cref.HELD), (cref.HELD, 0)):
        assert 20 < int(((e & bits) == value).sum()) < e.shape[0], (bits, value)
    a = _scene('exact_a')[0]
    assert all(v[0] == 1 and v[1] == 0 for v in a.rec.values()) and a.num_voxels > 1000


@pytest.mark.parametrize('name', COMPARE_NAMES)
def test_compare_host_build_equals_the_restatement(host_exe, tmp_path, name):
    got, want = _host_compare(host_exe, tmp_path, name), _restatement(name)
    assert got['counters'] == _flat(want['counters']), name
    for side in ('self', 'other'):
        _assert_columns(got[side], want[side], (name, side))
        c = want['counters'][side]
        assert c['kept'] == got[side]['status'].shape[0] and c['same'] <= c['held'] and c['only'] + c['near'] <= c['kept'] + c['same'], name


def test_compare_relations(host_exe, tmp_path):
    count = lambda name: _host_compare(host_exe, tmp_path, name)['counters']
    # rows, kept, same, held, near, only per side
    assert count('below') == [37, 37, 0, 0, 0, 37, 30, 30, 0, 0, 0, 30] and count('rows_0_0') == [0] * 12
    assert count('rows_0_65') == [0, 0, 0, 0, 0, 0, 65, 65, 0, 0, 0, 65] and count('rows_65_0') == [65, 65, 0, 0, 0, 65, 0, 0, 0, 0, 0, 0]
    c = count('contained')
    assert c[:4] == [60, 60, 16, 16] and c[6:10] == [16, 16, 16, 16] and c[11] == 0
    for name in ('identical', 'self'):                                           # every row SAME | HELD | NEAR at distance 0, in its own row
        got = _host_compare(host_exe, tmp_path, name)
        n = got['counters'][0]
        assert got['counters'] == [n, n, n, n, n, 0] * 2, name
        for side in ('self', 'other'):
            s = got[side]
            assert (s['status'] == 7).all() and (s['distance'] == 0.0).all() and np.array_equal(s['same_row'], np.arange(n)) and np.array_equal(s['row'], s['same_row'])
    for name, has_a, has_b in (('sidecar_a', True, False), ('sidecar_b', False, True), ('no_sidecar', False, False), ('sidecar_both', True, True)):
        got = _host_compare(host_exe, tmp_path, name)                            # a side reports the OTHER map's ray counts; 0 without a sidecar there
        assert (got['self']['pierced'].any() == has_b) and (got['other']['pierced'].any() == has_a), name
        assert not got['self']['pierced'][(got['self']['status'] & cref.HELD) == 0].any(), name


@pytest.mark.parametrize('name', SELECT_NAMES)
def test_select_host_build_equals_the_restatement(host_exe, tmp_path, name):
    scene, rule, invert, min_count, mmf = SELECT_CASES[name]
    r, p = _scene(scene)
    want, wp, counters = cref.select(r, p, _mask(name), invert, min_count, mmf)
    got = _host_select(host_exe, tmp_path, name)
    assert got['counters'] == counters, name
    if rule in ('short', 'long'):                                                # refused: the driver asserts that every output row is still poison
        assert counters[0] == cref.BAD_MASK and got['state'] == [0x5b5b5b5b5b5b5b5b] * 8 and got['keys'].shape[0] == 0, name
        return
    assert counters[0] == cref.OK and got['state'] == [counters[3]] + [0] * 7, name
    ah.assert_tables(got, ah.as_tables(want, wp), name)
    if name == 'all':
        ah.assert_tables(got, ah.as_tables(r, p), name)
    if name == 'none':
        assert counters[3] == 0
    if name == 'sheet':
        assert counters == [0, 76661, 76661, 25554]


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_compare_workspace_bytes', 'pcacc_accum_compare', 'pcacc_accum_select_workspace_bytes', 'pcacc_accum_select'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C13. ' in header and len(native._PROTOTYPES['pcacc_accum_compare']) == 29 and len(native._PROTOTYPES['pcacc_accum_select']) == 22
    for word, value in (('COMPARE_SAME', 1), ('COMPARE_HELD', 2), ('COMPARE_NEAR', 4), ('COMPARE_COUNTERS', 12), ('COMPARE_SIDE_COUNTERS', 6),
                        ('COMPARE_ROWS', 0), ('COMPARE_KEPT', 1), ('COMPARE_N_SAME', 2), ('COMPARE_N_HELD', 3), ('COMPARE_N_NEAR', 4), ('COMPARE_N_ONLY', 5),
                        ('SELECT_COUNTERS', 4), ('SELECT_STATUS', 0), ('SELECT_ROWS', 1), ('SELECT_KEPT', 2), ('SELECT_SELECTED', 3), ('SELECT_OK', 0),
                        ('SELECT_BAD_MASK', 1)):
        assert ('#define PCACC_%s %d' % (word, value)) in header and getattr(native, word) == value, word
    assert (cref.SAME, cref.HELD, cref.NEAR) == (native.COMPARE_SAME, native.COMPARE_HELD, native.COMPARE_NEAR)
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = open(os.path.join(csrc, 'accum_compare.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_prune.h"', '#include "accum_query.h"']        # nothing of HIP
    assert all(s in text for s in ('accum_lower_bound(', 'accr_match(', 'accn_centroid(', 'accum_unkey(', 'accum_field(', 'accn_index('))
    body = text.split('#pragma once')[1]
    assert not any(s in body for s in ('32768', '1048576', '65536', 'ACC_FIXED_ONE', 'ACC_IDX_BIAS', '0.9'))      # no bound and no helper restated
    hip = open(os.path.join(csrc, 'accum_compare.hip')).read()
    assert all(s in hip for s in ('pcacc_scan_i32(', 'accum_wave_count(', 'accum_tables_overlap(', 'accn_rows_launch(', 'accn_rows_ws_carve(', 'accr_move_row('))
    assert hip.count('__global__') == 3 and hip.count('hipLaunchKernelGGL(accd_side_kernel') == 2          # one kernel body serves both directions
    assert 'accum_compare.hip' in open(os.path.join(csrc, 'Makefile')).read()
    a, b = AccumulatedCloud(0.1, 'cpu', 64), AccumulatedCloud(0.2, 'cpu', 64)
    for call in (a.compare, a.difference):
        with pytest.raises(ValueError, match=r'regrid\(\)'):                     # before any call: the device is never asked
            call(b)
        with pytest.raises(ValueError, match=r'regrid\(\)'):
            call(AccumulatedCloud(np.nextafter(0.1, 1.0), 'cpu', 64))            # float equality
        for bad in (5, None, 'map', (a,)):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (dict(max_distance=0.0), dict(max_distance=0.11), dict(max_distance=float('nan')), dict(min_count=0)):
            with pytest.raises(ValueError):
                call(AccumulatedCloud(0.1, 'cpu', 64), **bad)
        with pytest.raises(native.NativeError):                                  # there is no CPU path
            call(AccumulatedCloud(0.1, 'cpu', 64))
    assert 'pose' not in a.compare.__code__.co_varnames
    for bad in (None, [1, 0], torch.zeros(3), torch.zeros(2, 2, dtype=torch.bool)):
        with pytest.raises(ValueError):
            a.select(bad)
    with pytest.raises(native.NativeError):
        a.select(torch.zeros(0, dtype=torch.bool))
    cpu = (torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(native.NativeError):
        native.accum_compare(cpu, 0, None, cpu, 0, None, 0.1, 0.1, 1, None)
    with pytest.raises(native.NativeError):
        native.accum_select(cpu, 0, None, 1, None, torch.zeros(0, dtype=torch.uint8), False, tuple(t.clone() for t in cpu), None,
                            torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64))


def test_bad_arguments_return_before_anything_is_launched():
    """Every PCACC_E_ARG is decided on the host before the first launch, so the entry points can be asked without a GPU: the addresses below are
    never used.  (test_bad_arguments_launch_nothing_gpu asks again with real tables and looks at them afterwards.)"""
    from pcaccumulation_amd import native
    lib, big = native.lib(), (1 << 30) + 1
    need = ctypes.c_size_t(0)
    assert lib.pcacc_accum_compare_workspace_bytes(5, 7, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pcacc_accum_compare_workspace_bytes(0, 0, ctypes.byref(need)) == 0 and need.value > 0
    for ma, mb in ((-1, 0), (0, -1), (big, 0), (0, big)):
        assert lib.pcacc_accum_compare_workspace_bytes(ma, mb, ctypes.byref(need)) == -1
    assert lib.pcacc_accum_compare_workspace_bytes(1, 1, None) == -1
    assert lib.pcacc_accum_select_workspace_bytes(9, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pcacc_accum_select_workspace_bytes(-1, ctypes.byref(need)) == -1 and lib.pcacc_accum_select_workspace_bytes(big, ctypes.byref(need)) == -1
    p = 4096                                                                     # stands for a table; never dereferenced
    good = dict(ak=p, aa=p, ap=None, acap=8, ma=5, bk=p, ba=p, bp=None, bcap=8, mb=5, vs=0.1, dist=0.1, min_count=1, use_f=0, f=0.0,
                o=[p] * 10, counters=p, ws=p, ws_bytes=1 << 20)
    def compare(**kw):
        a = dict(good, **kw)
        o = a['o']
        return lib.pcacc_accum_compare(a['ak'], a['aa'], a['ap'], a['acap'], a['ma'], a['bk'], a['ba'], a['bp'], a['bcap'], a['mb'], a['vs'], a['dist'],
                                       a['min_count'], a['use_f'], a['f'], o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], a['counters'],
                                       a['ws'], a['ws_bytes'], None)
    bad = [dict(ma=9), dict(ma=-1), dict(mb=9), dict(mb=-1), dict(acap=big, ma=5), dict(bcap=big), dict(min_count=0), dict(min_count=-3),
           dict(vs=0.0), dict(vs=-0.1), dict(vs=float('nan')), dict(vs=float('inf'), dist=1.0), dict(dist=0.0), dict(dist=-0.05), dict(dist=float('nan')),
           dict(dist=float('inf')), dict(dist=np.nextafter(0.1, 1.0)), dict(ak=None), dict(aa=None), dict(bk=None), dict(ba=None), dict(counters=None),
           dict(ws=None)]
    bad += [dict(o=[None if k == j else p for k in range(10)]) for j in range(10)]
    for kw in bad:
        assert compare(**kw) == -1, kw
    assert compare(ws_bytes=16) == -2
    sgood = dict(ik=p, ia=p, is_=p, ip=None, icap=8, m=5, min_count=1, mask=p, mask_rows=5, ok=p + 4096, oa=p + 8192, os_=p + 16384, op=None, ocap=8,
                 counters=p, state=p, ws=p, ws_bytes=1 << 20)
    def select(**kw):
        a = dict(sgood, **kw)
        return lib.pcacc_accum_select(a['ik'], a['ia'], a['is_'], a['ip'], a['icap'], a['m'], a['min_count'], 0, 0.0, a['mask'], a['mask_rows'], 0,
                                      a['ok'], a['oa'], a['os_'], a['op'], a['ocap'], a['counters'], a['state'], a['ws'], a['ws_bytes'], None)
    far = 1 << 40                                                                # tables that share nothing
    sgood.update(ik=far, ia=2 * far, is_=3 * far, ok=4 * far, oa=5 * far, os_=6 * far)
    for kw in (dict(m=9), dict(m=-1), dict(icap=big), dict(ocap=big), dict(ocap=4), dict(min_count=0), dict(mask_rows=-1), dict(mask=None), dict(ik=None),
               dict(ia=None), dict(is_=None), dict(ok=None), dict(oa=None), dict(os_=None), dict(ip=7 * far), dict(counters=None), dict(state=None),
               dict(ws=None), dict(ok=far), dict(oa=2 * far + 8), dict(os_=far + 8 * 7), dict(ok=3 * far + 8 * 7), dict(ip=7 * far, op=far + 8)):
        assert select(**kw) == -1, kw
    assert select(ws_bytes=16) == -2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
def _device_cloud(r, pierced):
    """The restatement's map and {key: rays} dict as an AccumulatedCloud on the device."""
    return ah.device_cloud(r, None if pierced is None else mref.aligned(pierced, r.records()[0]), np.arange(5, dtype=np.int64) + r.num_voxels)


def _assert_same_map(a, b, what):
    n = b.num_voxels
    assert a.num_voxels == n and a.voxel_size == b.voxel_size, what
    for x, y in zip(a._cur, b._cur):
        assert torch.equal(x[..., :n], y[..., :n]), what
    assert (a._pierced is None) == (b._pierced is None), what
    if a._pierced is not None:
        assert a._pierced.shape[0] == a.capacity and torch.equal(a._pierced[:n], b._pierced[:n]), what


def _assert_device_equals_host(m, host, what):
    t = lambda a: torch.from_numpy(a).to(DEV)
    n = host['keys'].shape[0]
    assert m.num_voxels == n, what
    keys, acc, stamps = m._cur
    assert torch.equal(keys[:n], t(host['keys'])) and torch.equal(acc[:, :n], t(host['acc'])) and torch.equal(stamps[:, :n], t(host['stamps'])), what
    assert (m._pierced is None) == (host['pierced'] is None), what
    if host['pierced'] is not None:
        assert m._pierced.shape[0] == m.capacity and torch.equal(m._pierced[:n], t(host['pierced'])), what


def _host_columns(side):
    return {name: side[name].cpu().numpy() for name, _ in COLUMNS}


@pytest.mark.gpu
@pytest.mark.parametrize('name', COMPARE_NAMES)
def test_compare_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """Claims 1, 3 and 4: columns and counters of both sides; the rows are extract()'s under the same filter; a sidecar on one side, both, neither."""
    a, b, dist, min_count, mmf = COMPARE_CASES[name]
    host = _host_compare(host_exe, tmp_path, name)
    A = _device_cloud(*_scene(a))
    B = A if b is None else _device_cloud(*_scene(b))
    snap_a, snap_b = ah.snapshot(A), ah.snapshot(B)
    got = A.compare(B, dist, min_count, mmf)
    assert _flat(got['counters']) == host['counters'] and all(type(v) is int for c in got['counters'].values() for v in c.values()), name
    for side, m in (('self', A), ('other', B)):
        assert all(t.device == m._cur[0].device for t in got[side].values()), name
        _assert_columns(_host_columns(got[side]), host[side], (name, side))
        assert got[side]['status'].shape[0] == m.extract(min_count, mmf)['count'].shape[0] == got['counters'][side]['kept'], name
    ah.assert_unchanged(A, snap_a, name)
    ah.assert_unchanged(B, snap_b, name)
    if name == 'filter':                                                         # same_row and row index the OTHER side's extract under the filter
        s, other = got['self'], B.extract(min_count, mmf)
        same, near = (s['status'] & cref.SAME) != 0, (s['status'] & cref.NEAR) != 0
        assert bool(((s['status'] & (cref.HELD | cref.SAME)) == cref.HELD).any())            # HELD without SAME occurs
        own = A.extract(min_count, mmf)
        assert torch.equal(other['coords'][s['same_row'][same].long()], own['coords'][same])
        assert int((other['coords'][s['row'][near].long()] - own['coords'][near]).abs().max()) <= 1
        assert int(other['count'].min()) >= 2 and int(own['count'].min()) >= 2
    again = A.compare(B, dist, min_count, mmf)                                   # a second run gives the same bits
    for side in ('self', 'other'):
        _assert_columns(_host_columns(again[side]), host[side], (name, side, 'again'))


@pytest.mark.gpu
def test_compare_is_query_gpu():
    """Claim 2: a map of one point per voxel, exact in float32 and in fixed point, compared with another map, is that map queried at its points."""
    from pcaccumulation_amd import native
    A, B = _device_cloud(*_scene('exact_a')), _device_cloud(*_scene('exact_b'))
    for dist, mmf in ((0.05, 0.0), (0.1, 0.0), (0.09, None)):
        points = A.extract(1, mmf)['points']
        assert points.shape[0] == A.num_voxels
        s, q = A.compare(B, dist, 1, mmf)['self'], B.query(points, None, dist, 1, mmf)
        assert torch.equal(s['row'], q['row']) and torch.equal(s['distance'].view(torch.int64), q['distance'].view(torch.int64))
        assert torch.equal(s['pierced'], q['pierced'])
        for mine, theirs in ((cref.NEAR, native.QUERY_MATCHED), (cref.HELD, native.QUERY_OCCUPIED), (cref.SAME, native.QUERY_KEPT)):
            assert torch.equal((s['status'] & mine) != 0, (q['status'] & theirs) != 0)
        assert not bool((q['status'] & native.QUERY_INVALID).any()) and 0 < int(((s['status'] & cref.NEAR) != 0).sum()) < points.shape[0]
        assert bool(s['pierced'].any())


@pytest.mark.gpu
def test_compare_agrees_with_merge_gpu():
    """Claim 5, on add-built maps at min_count = 1."""
    A, B = ah.added((1, 3)), ah.added((2, 4))
    snap_a, snap_b = ah.snapshot(A), ah.snapshot(B)
    got = A.compare(B)
    ah.assert_unchanged(A, snap_a, 'compare modifies nothing')
    ah.assert_unchanged(B, snap_b, 'compare modifies nothing')
    res = A.copy().merge(B)
    ca, cb = got['counters']['self'], got['counters']['other']
    assert ca['same'] == cb['same'] == res['shared'] > 0 and cb['kept'] - cb['held'] == res['new'] > 0
    assert (ca['rows'], cb['rows']) == (A.num_voxels, B.num_voxels) == (ca['kept'], cb['kept']) and ca['held'] == ca['same'] and cb['held'] == cb['same']
    own = A.compare(A)
    n = A.num_voxels
    for side in ('self', 'other'):
        s = own[side]
        assert bool((s['status'] == 7).all()) and bool((s['distance'] == 0.0).all()), side
        assert torch.equal(s['same_row'], torch.arange(n, dtype=torch.int32, device=DEV)) and torch.equal(s['row'], s['same_row']), side
        assert own['counters'][side] == dict(rows=n, kept=n, same=n, held=n, near=n, only=0)
    ah.assert_unchanged(A, snap_a, 'compare(self)')
    empty = ah.added(())                                                           # a map that never saw an add
    got = A.compare(empty)
    assert got['counters']['self'] == dict(rows=n, kept=n, same=0, held=0, near=0, only=n) and got['counters']['other'] == dict.fromkeys(cref.SIDE, 0)
    assert got['other']['status'].shape[0] == 0 and bool((got['self']['row'] == -1).all()) and bool(torch.isinf(got['self']['distance']).all())


@pytest.mark.gpu
@pytest.mark.parametrize('name', SELECT_NAMES)
def test_select_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    from pcaccumulation_amd import native
    scene, rule, invert, min_count, mmf = SELECT_CASES[name]
    host = _host_select(host_exe, tmp_path, name)
    A = _device_cloud(*_scene(scene))
    snap = ah.snapshot(A)
    mask = torch.from_numpy(_mask(name)).to(DEV)
    if rule in ('short', 'long'):                                                # a mask of the wrong length: the method raises,
        with pytest.raises(ValueError, match=r'one entry per row of extract\(\) under the same filter \(%d rows\)' % host['counters'][2]):
            A.select(mask, invert, min_count, mmf)
        out = tuple(torch.full_like(t, 7) for t in A._cur)                       # and the direct call leaves tables and state untouched
        pout = None if A._pierced is None else torch.full_like(A._pierced, 7)
        counters, state = torch.full((4,), 7, dtype=torch.int64, device=DEV), torch.full((8,), 7, dtype=torch.int64, device=DEV)
        native.accum_select(A._cur, A.num_voxels, A._pierced, min_count, mmf, mask, invert, out, pout, counters, state)
        assert counters.tolist() == host['counters'] and counters.tolist()[0] == native.SELECT_BAD_MASK
        assert state.tolist() == [7] * 8 and all(bool((t == 7).all()) for t in out + (() if pout is None else (pout,)))
        ah.assert_unchanged(A, snap, name)
        return
    got = A.select(mask.bool() if name == 'rows65' else mask, invert, min_count, mmf)
    ah.assert_unchanged(A, snap, name)
    _assert_device_equals_host(got, host, name)
    assert got._state.tolist() == host['state'] and got.dropped == 0 and got.capacity == A.capacity and got.voxel_size == A.voxel_size, name
    assert got is not A and got._cur[0].data_ptr() != A._cur[0].data_ptr()
    if A._pierced is not None:
        assert torch.equal(got._pierce_counters, A._pierce_counters) and got._pierce_counters is not A._pierce_counters
    keep = (mask != 0) != invert                                                 # select(mask).extract() is extract() indexed by the mask
    mine, whole = got.extract(), A.extract(min_count, mmf)
    for k in whole:
        assert torch.equal(mine[k], whole[k][keep]), (name, k)
    small = A.select(mask, invert, min_count, mmf, capacity=max(A.num_voxels, 1))            # the smallest capacity the call takes
    _assert_same_map(small, got, name)
    with pytest.raises(ValueError):
        A.select(mask, invert, min_count, mmf, capacity=A.num_voxels - 1)


@pytest.mark.gpu
def test_select_is_prune_and_its_halves_merge_back_gpu():
    for scene in ('dense_b', 'dense'):                                           # with and without a sidecar
        A = _device_cloud(*_scene(scene))
        snap = ah.snapshot(A)
        kept = A.extract(2)['count'].shape[0]
        got = A.select(torch.ones(kept, dtype=torch.bool, device=DEV), min_count=2)
        want = A.copy()
        want.prune(min_count=2)
        _assert_same_map(got, want, scene)
        assert got.num_voxels == kept < A.num_voxels
        mask = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, A.num_voxels) < 0.4).to(DEV)
        x, y = A.select(mask), A.select(mask, invert=True)
        assert x.num_voxels + y.num_voxels == A.num_voxels and 0 < x.num_voxels < A.num_voxels
        x.merge(y)
        _assert_same_map(x, A, scene)
        ah.assert_unchanged(A, snap, scene)


@pytest.mark.gpu
def test_difference_gpu():
    from pcaccumulation_amd import native
    for a, b, dist, min_count, mmf in (SHEET_CASES['sheet_half'], COMPARE_CASES['filter'], COMPARE_CASES['sidecar_both']):
        A, B = _device_cloud(*_scene(a)), _device_cloud(*_scene(b))
        snap_a, snap_b = ah.snapshot(A), ah.snapshot(B)
        got = A.difference(B, dist, min_count, mmf)
        c = A.compare(B, dist, min_count, mmf)
        by_hand = A.select((c['self']['status'] & (native.COMPARE_SAME | native.COMPARE_NEAR)) == 0, min_count=min_count, max_moving_fraction=mmf)
        _assert_same_map(got, by_hand, a)
        assert got.num_voxels == c['counters']['self']['only'] and 0 < got.num_voxels < A.num_voxels, a
        ah.assert_unchanged(A, snap_a, a)
        ah.assert_unchanged(B, snap_b, a)
    assert A.difference(A).num_voxels == 0


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    A, B = _device_cloud(*_scene('rays_a')), _device_cloud(*_scene('rays_b'))
    assert (A.num_voxels, A.capacity, B.num_voxels, B.capacity) == (70, 128, 70, 128)
    snap_a, snap_b = ah.snapshot(A), ah.snapshot(B)
    fresh = lambda rows: {name: torch.full((rows,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in native.COMPARE_FIELDS}
    oa, ob, cc = fresh(70), fresh(70), torch.full((12,), 7, dtype=torch.int64, device=DEV)
    good = dict(tables_a=A._cur, ma=70, pierced_a=A._pierced, tables_b=B._cur, mb=70, pierced_b=B._pierced, voxel_size=0.1, max_distance=0.1, min_count=1,
                max_moving_fraction=None, out_a=oa, out_b=ob, counters=cc)
    for bad in (dict(ma=129, out_a=fresh(129)), dict(ma=-1, out_a=fresh(0)), dict(mb=129, out_b=fresh(129)), dict(mb=-1, out_b=fresh(0)), dict(min_count=0),
                dict(voxel_size=0.0), dict(voxel_size=float('nan')), dict(voxel_size=float('inf')), dict(max_distance=0.0), dict(max_distance=float('nan')),
                dict(max_distance=0.1000001), dict(max_distance=-0.05)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_compare(**dict(good, **bad))
    out = tuple(torch.full_like(t, 7) for t in A._cur)
    pout = torch.full_like(A._pierced, 7)
    small = tuple(t[..., :69].contiguous() for t in out)
    sc, state = torch.full((4,), 7, dtype=torch.int64, device=DEV), torch.full((8,), 7, dtype=torch.int64, device=DEV)
    mask = torch.ones(70, dtype=torch.uint8, device=DEV)
    sgood = dict(tables_in=A._cur, m=70, pierced_in=A._pierced, min_count=1, max_moving_fraction=None, mask=mask, invert=False, tables_out=out,
                 pierced_out=pout, counters=sc, state=state)
    for bad in (dict(tables_out=A._cur), dict(pierced_out=A._pierced), dict(tables_out=(out[0], A._cur[1], out[2])), dict(tables_out=(out[0], out[1], A._cur[2])),
                dict(tables_out=(A._cur[0], out[1], out[2])), dict(tables_out=small, pierced_out=pout[:69].contiguous()), dict(m=129), dict(m=-1),
                dict(min_count=0), dict(pierced_out=None)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_select(**dict(sgood, **bad))
    torch.cuda.synchronize()
    ah.assert_unchanged(A, snap_a, 'bad arguments')
    ah.assert_unchanged(B, snap_b, 'bad arguments')
    assert all(bool((t == 7).all()) for t in out + small + (pout, cc, sc, state) + tuple(oa.values()) + tuple(ob.values()))    # nothing was written
    native.accum_compare(**dict(good, ma=0, mb=0, out_a=fresh(0), out_b=fresh(0)))           # ma = mb = 0: the zero counters, nothing else
    assert cc.tolist() == [0] * 12
    native.accum_select(**dict(sgood, m=0, mask=mask[:0]))                       # m = 0: the counters and the state of an empty map, no table
    assert sc.tolist() == [0, 0, 0, 0] and state.tolist() == [0] * 8 and all(bool((t == 7).all()) for t in out + (pout,))
