"""The (x, y) columns of the accumulated scene cloud, their local ground, heights above it and bird's-eye-view rasters (include/pcacc.h C17, DESIGN.md
section 9q): AccumulatedCloud.columns / ground_mask / split_ground / bev.

Every result is an integer, or a float that one fixed sequence of IEEE operations gives, so every claim is an equality of integers or bits; no tolerance
appears anywhere.
  CPU   the g++ build of csrc/accum_columns.h (tests/accum_columns_host_driver.cpp, every table index asserted, poison behind the rows in use and in every
        output, every output element written once) against the plain-Python restatement on dicts keyed by (x, y) (tests/accumulate_columns_reference.py:
        no keys, no sorted list, no scan); the capability scene (a ramp with boxes whose ground is occluded and a canopy) on the restatement alone;
  GPU   both entry points against the g++ build on the same cases, identities that tie the tables to extract() and records(), split_ground() against
        merge() (C12), bev() against a numpy scatter of columns(), a life cycle against the restatement, the model forward, and the argument checks."""
import os

import numpy as np
import pytest
import torch

import accumulate_columns_reference as cref
import accumulate_helpers as ah
import accumulate_prune_reference as rref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

FILTER = dict(min_count=2, max_moving_fraction=0.5)
TOP = cref.MAX_HEIGHT                                                               # a band above every voxel of every scene but `edge`


# ---- scenes: a ReferenceMap each, built once and never modified ------------------------------------------------------------------------------------------
TIE = [(0, 0, 4), (0, 0, 6), (0, 1, 4), (1, 0, 5), (1, 1, 9)]                       # two neighbouring columns with equal z_low = 4, and two above them
# the filter scene: (0, 0) has one voxel of one point, (2, 0) a voxel of one point below one of two: min_count = 2 removes column (0, 0) and lifts (2, 0)
FILTERED = {(0, 0, 0): (1, 0, 0, 0), (1, 0, 3): (2, 0, 1, 2), (1, 0, 4): (2, 2, 3, 5), (2, 0, 1): (1, 0, 0, 0), (2, 0, 5): (2, 0, 4, 4), (2, 1, 7): (3, 1, 2, 9)}


def _edge_voxels():
    """The four corner columns of the grid with voxels at z = -2^20 and 2^20 - 1; and four columns at z_low = 10 on the four edges, each with the decoy
    where a y field that wrapped (or an x - R below the grid) would look: one voxel at z = -2^20, so a decoy taken for a neighbour wins at once."""
    E = EDGE
    vox = [(x, y, z) for x in (-E, E - 1) for y in (-E, E - 1) for z in (-E, E - 1)]
    vox += [(100, E - 1, 10), (100, E - 1, E - 1), (101, -E, -E)]                   # (101, -2^20) follows (100, 2^20 - 1) directly in the list
    vox += [(200, -E, 10), (199, E - 1, -E)]                                        # y - R below the grid aliases (199, 2^20 - k)
    vox += [(-E, 50, 10), (-E, 53, 12), (E - 1, 300, 10), (E - 1, 296, 8), (E - 9, 300, 3), (E - 10, 300, 1)]    # x - R / x + R leave the grid; 9 and 10 away
    return vox


def _capability():
    """0.1 m voxels.  A 40 x 40-column ramp rising 0.05 m per column in x, one point per column with +-3 cm xy and +-2 cm z noise; three 4 x 4-column boxes
    with NO ramp voxel beneath them, at local heights 3..14 voxels; a 10 x 10 canopy 30 voxels above the ramp.  -> points, {voxel: label}."""
    rs = np.random.RandomState(1017)
    boxes, canopy = [(5, 5), (20, 12), (30, 28)], (10, 25)
    under = {(bx + a, by + b) for bx, by in boxes for a in range(4) for b in range(4)}
    pts, label = [], {}
    for i in range(40):
        zr = i // 2                                                                 # 0.05 i + 0.025 +- 0.02 m: the ramp's voxel of column i
        for j in range(40):
            if (i, j) in under:
                for h in range(3, 15):
                    pts.append(((i + 0.5) * 0.1, (j + 0.5) * 0.1, (zr + h + 0.5) * 0.1))
                    label[(i, j, zr + h)] = 'box'
                continue
            pts.append(((i + 0.5) * 0.1 + rs.uniform(-0.03, 0.03), (j + 0.5) * 0.1 + rs.uniform(-0.03, 0.03), 0.05 * i + 0.025 + rs.uniform(-0.02, 0.02)))
            label[(i, j, zr)] = 'ramp'
            if canopy[0] <= i < canopy[0] + 10 and canopy[1] <= j < canopy[1] + 10:
                pts.append(((i + 0.5) * 0.1, (j + 0.5) * 0.1, (zr + 30 + 0.5) * 0.1))
                label[(i, j, zr + 30)] = 'canopy'
    return np.array(pts, np.float32), label


_scenes = {}


def _build_scene(name):
    if name.startswith('rows'):
        return ah.records(0.1, ah.random_rows(int(name[4:]), 100 + int(name[4:]))[0])
    if name == 'dense11':
        return ah.rows([tuple(int(v) for v in c) for c in ah.block(-5, 6)], 3)[0]
    if name == 'tower':                                                             # one run of 300 rows: the walk of one lane across waves
        return ah.rows([(0, 0, z) for z in range(-100, 200)] + [(0, 1, 57)], 5)[0]
    if name == 'flat300':                                                           # every row a head: 300 columns in one x, 257 in the next
        return ah.rows([(0, y, (7 * y) % 5) for y in range(300)] + [(1, y, (3 * y) % 7) for y in range(257)], 6)[0]
    if name == 'tie':
        return ah.rows(TIE, 7)[0]
    if name == 'edge':
        return ah.rows(_edge_voxels(), 8, vs=0.01)[0]
    if name == 'filtered':
        return ah.records(0.1, FILTERED)
    assert name == 'capability'
    return ah.points_map(0.1, [(_capability()[0], None, 0)])


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


# ---- cases: a scene and the arguments of one columns() call; the windows of bev() follow from the restated columns ---------------------------------------
RADII = (0, 1, 2, 8)
SETTINGS = {0: dict(thickness=0, band=(0, 0)), 1: dict(thickness=3, band=(2, 20)), 2: dict(thickness=1, band=(2, 20)), 8: dict(thickness=0, band=(TOP, TOP))}


def _cases():
    cases = {}
    for scene in ('rows0', 'rows1', 'rows65', 'rows343', 'dense11', 'tower', 'flat300', 'tie', 'edge', 'filtered'):
        for R in RADII:
            cases['%s_r%d' % (scene, R)] = (scene, dict(ground_radius=R, **SETTINGS[R]))
    cases['dense11_r2_thick3_band0'] = ('dense11', dict(ground_radius=2, thickness=3, band=(0, 0)))
    cases['tower_r1_band_wide'] = ('tower', dict(ground_radius=1, thickness=0, band=(0, TOP)))
    cases['edge_r8_band_all'] = ('edge', dict(ground_radius=8, thickness=TOP, band=(0, TOP)))
    cases['filtered_r1_min2'] = ('filtered', dict(ground_radius=1, thickness=1, band=(2, 20), min_count=2))
    cases['filtered_r1_static'] = ('filtered', dict(ground_radius=1, thickness=1, band=(2, 20), max_moving_fraction=0.5))
    cases['rows343_r2_filtered'] = ('rows343', dict(ground_radius=2, thickness=1, band=(1, 3), **FILTER))
    cases['rows343_r2_all_filtered'] = ('rows343', dict(ground_radius=2, thickness=1, band=(2, 20), min_count=7))      # random_rows counts 1..6
    cases['flat300_r8_filtered'] = ('flat300', dict(ground_radius=8, thickness=1, band=(1, 4), min_count=3))           # heads move off the boundaries
    cases['capability_r2'] = ('capability', dict(ground_radius=2, thickness=1, band=(2, 20)))
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)
_restated = {}


def _restate(name):
    if name not in _restated:
        scene, args = CASES[name]
        _restated[name] = cref.columns(_scene(scene), **args)
    return _restated[name]


def _windows(name):
    """[(origin, shape)]: first a window wholly empty; then the bounding box (where it has at most 2^16 pixels: all scenes but `edge`), a window half off
    the map, 1 x 1 windows on a column and beside the map, and windows that touch and cross the grid edge at 2^20 - 1 and at -2^20."""
    cols = _restate(name)
    (x0, y0), (H, W) = cref.bounding_box(cols)
    out = [((x0 + 5000, y0 - 7000), (3, 2))]
    if H * W <= 1 << 16:
        out += [((x0, y0), (H, W)), ((x0 - (W + 1) // 2, y0 + H // 2), (H, W)), ((x0 + 3, y0 - 2), (min(H, 5), min(W, 7)))]
    out += [((x0, y0), (1, 1)), ((x0 - 1, y0 - 1), (1, 1)), ((EDGE - 3, EDGE - 4), (7, 6)), ((-EDGE - 2, -EDGE - 1), (3, 4))]
    if cols['n_columns']:
        x, y = cols['xy'][cols['n_columns'] // 2].tolist()
        out += [((x, y), (1, 1)), ((x - 1, y - 2), (4, 3))]
    return out


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_columns_host_driver', 'columns_host')
HOST_COLUMNS = [('key', np.int64)] + [(f, cref.DTYPES[f]) for f in cref.COLUMN_FIELDS]


def _run_host(exe, tmp_path, tag, r, windows, ground_radius, thickness, band, min_count=1, max_moving_fraction=None, spare=3):
    keys, acc, stamps = r.records()
    m = keys.shape[0]
    head = [m, m + spare, min_count, 0 if max_moving_fraction is None else 1, ground_radius, thickness, band[0], band[1], len(windows)]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array([0.0 if max_moving_fraction is None else max_moving_fraction], np.float64),
                        ah.map_bytes(keys, acc, stamps), np.array([[o[0], o[1], s[1], s[0]] for o, s in windows], np.int64).reshape(-1, 4))
    kept, C = (int(v) for v in np.frombuffer(raw, np.int64, 2, 40))
    out, off = ah.unpack(raw, 56, [(f, d, (C, 2) if f == 'xy' else (C,)) for f, d in HOST_COLUMNS] + [(f, cref.DTYPES[f], (kept,)) for f in cref.ROW_FIELDS])
    images = []
    for _, (H, W) in windows:
        image, off = ah.unpack(raw, off, [(f, cref.DTYPES[f], (H, W)) for f in cref.BEV_FIELDS])
        images.append(image)
    assert off == len(raw)
    return dict(out, counters=np.frombuffer(raw, np.int64, 5).tolist(), kept=kept, n_columns=C, images=images)


_hosted = {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, args = CASES[name]
        _hosted[name] = _run_host(exe, tmp_path, name, _scene(scene), _windows(name), **args)
    return _hosted[name]


def _assert_same(got, want, what, fields=cref.COLUMN_FIELDS + cref.ROW_FIELDS):
    assert list(got['counters']) == list(want['counters']), (what, got['counters'], want['counters'])
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape, want[f].shape)
        assert np.array_equal(ah.bits(got[f]), ah.bits(want[f])), (what, f, np.flatnonzero((ah.bits(got[f]) != ah.bits(want[f])).reshape(got[f].shape[0], -1).any(1))[:5])


def _assert_same_image(got, want, what):
    for f in cref.BEV_FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(ah.bits(got[f]), ah.bits(want[f])), (what, f)


def _column_keys(xy):
    return ((xy[:, 0].astype(np.int64) + EDGE) << 21) | (xy[:, 1].astype(np.int64) + EDGE)


# ---- CPU: host build == restatement ------------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    assert [_scene('rows%d' % m).num_voxels for m in (0, 1, 65, 343)] == [0, 1, 65, 343] and _scene('dense11').num_voxels == 1331
    tower = _restate('tower_r1')
    assert tower['voxels'].tolist() == [300, 1] and tower['first_row'].tolist() == [0, 300] and tower['counters'][4] == 1     # the neighbour borrows
    flat = _restate('flat300_r0')
    assert flat['n_columns'] == flat['kept'] == 557 and flat['first_row'].tolist() == list(range(557)) and flat['counters'][4] == 0
    heads = set(_restate('flat300_r8_filtered')['first_row'].tolist())
    assert 0 < _restate('flat300_r8_filtered')['kept'] < 557 and len(heads) > 257
    for boundary in (63, 64, 65, 256, 257):                                         # run heads on wave and workgroup boundaries
        assert boundary in set(flat['first_row'].tolist())
    assert _restate('rows343_r2_all_filtered')['kept'] == 0 < _restate('rows343_r2_filtered')['kept'] < 343
    edge = _restate('edge_r8')
    at = {tuple(xy): c for c, xy in enumerate(edge['xy'].tolist())}
    assert edge['z_low'].min() == -EDGE and edge['z_high'].max() == EDGE - 1 and edge['row_height'].max() == cref.MAX_HEIGHT
    assert edge['n_columns'] == len({v[:2] for v in _edge_voxels()}) == 14
    order = sorted(at)
    assert order[order.index((100, EDGE - 1)) + 1] == (101, -EDGE)                    # the decoy stands directly behind the column in the list


def test_a_tie_goes_to_the_lower_column():
    """Columns (0, 0) and (0, 1) both start at z = 4.  Rows of extract(): (0,0,4) (0,0,6) (0,1,4) (1,0,5) (1,1,9)."""
    got = _restate('tie_r1')
    assert got['xy'].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]] and got['z_low'].tolist() == [4, 4, 5, 9]
    assert got['ground_z'].tolist() == [4, 4, 4, 4] and got['ground_row'].tolist() == [0, 0, 0, 0] and got['ground_column'].tolist() == [0, 0, 0, 0]
    assert got['row_height'].tolist() == [0, 2, 0, 1, 5] and got['counters'] == [5, 4, 4, 2, 3]      # thickness 3, band (2, 20); three columns borrow
    alone = _restate('tie_r0')
    assert alone['ground_row'].tolist() == [0, 2, 3, 4] and alone['ground_column'].tolist() == [0, 1, 2, 3] and alone['counters'][4] == 0


def test_the_filter_removes_a_column_and_moves_a_ground():
    every, some = _restate('filtered_r1'), _restate('filtered_r1_min2')
    assert every['xy'].tolist() == [[0, 0], [1, 0], [2, 0], [2, 1]] and every['ground_z'].tolist() == [0, 0, 1, 1]
    assert some['xy'].tolist() == [[1, 0], [2, 0], [2, 1]] and some['z_low'].tolist() == [3, 5, 7] and some['ground_z'].tolist() == [3, 3, 3]
    assert some['kept'] == 4 and some['points'].tolist() == [4, 2, 3] and some['t_first'].tolist() == [1, 4, 2] and some['t_last'].tolist() == [5, 4, 9]
    static = _restate('filtered_r1_static')                                         # (1, 0, 4) is all moving
    assert static['voxels'].tolist() == [1, 1, 2, 1] and static['kept'] == 5


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want, got = _restate(name), _host(host_exe, tmp_path, name)
    assert (got['kept'], got['n_columns']) == (want['kept'], want['n_columns'])
    _assert_same(got, want, name)
    assert np.array_equal(got['key'], _column_keys(got['xy'])) and (np.diff(got['key']) > 0).all()
    c = got['counters']
    assert c == [got['kept'], got['n_columns'], int(got['row_is_ground'].sum()), int(got['band_voxels'].sum()),
                 int((got['ground_column'] != np.arange(got['n_columns'])).sum())]
    assert int(got['voxels'].sum()) == got['kept'] and (got['row_height'] >= 0).all()
    own = got['ground_row'][got['row_column']] == np.arange(got['kept'])             # a row that is the ground of its own column stands on itself
    assert own.sum() >= min(got['kept'], 1) and (got['row_height'][own] == 0).all() and (got['row_height_m'][own] == 0.0).all()


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_images_equal_the_restatement(host_exe, tmp_path, name):
    cols, got = _restate(name), _host(host_exe, tmp_path, name)
    windows = _windows(name)
    assert len(windows) >= 5 and len(got['images']) == len(windows)
    for (origin, shape), image in zip(windows, got['images']):
        _assert_same_image(image, cref.bev(cols, origin, shape), (name, origin, shape))
    if CASES[name][0] != 'edge':
        box = got['images'][1]                                                       # the bounding box holds every column once
        assert sorted(box['column'][box['column'] >= 0].tolist()) == list(range(cols['n_columns']))
        assert int(box['voxels'].sum()) == cols['kept']
    empty = got['images'][0]                                                         # the far window
    assert (empty['column'] == -1).all() and np.isnan(empty['elevation']).all() and np.isnan(empty['ground']).all() and (empty['voxels'] == 0).all()


def test_edge_windows_see_the_corner_columns(host_exe, tmp_path):
    got, windows = _host(host_exe, tmp_path, 'edge_r8'), _windows('edge_r8')
    at = {w: image for w, image in zip(windows, got['images'])}
    hi, lo = at[((EDGE - 3, EDGE - 4), (7, 6))], at[((-EDGE - 2, -EDGE - 1), (3, 4))]
    assert (hi['column'] >= 0).sum() == 1 and hi['column'][3, 2] >= 0 and (hi['column'][4:] == -1).all() and (hi['column'][:, 3:] == -1).all()
    assert (lo['column'] >= 0).sum() == 1 and lo['column'][1, 2] >= 0 and (lo['column'][0] == -1).all() and (lo['column'][:, :2] == -1).all()


# ---- CPU: the capability scene, on the restatement alone ---------------------------------------------------------------------------------------------------
def _capability_errors(cols, label, rows):
    ground = cols['row_is_ground'] != 0
    return sum(1 for j, (c, _) in enumerate(rows) if ground[j] != (label[c] == 'ramp'))


def test_the_ramp_is_the_ground_and_no_threshold_finds_it():
    """A slope with occluded ground under boxes: the local minimum over 5 x 5 columns separates it exactly; 3 x 3 columns do not reach under the boxes;
    no single z does."""
    r = _scene('capability')
    _, label = _capability()
    rows = cref.kept_rows(r)
    assert {c for c, _ in rows} == set(label) and len(rows) == 2228
    assert [sum(1 for v in label.values() if v == k) for k in ('ramp', 'box', 'canopy')] == [1552, 576, 100]
    cols = _restate('capability_r2')
    assert cols['n_columns'] == 1600 and cols['counters'][:4] == [2228, 1600, 1552, 576]
    assert _capability_errors(cols, label, rows) == 0                                # R = 2, thickness 1: the ground mask IS the ramp
    band = [c for j, (c, _) in enumerate(rows) if 2 <= cols['row_height'][j] <= 20]
    assert len(band) == 576 == int(cols['band_voxels'].sum()) and all(label[c] == 'box' for c in band)
    near = cref.columns(r, ground_radius=1, thickness=1)
    assert _capability_errors(near, label, rows) == 18                              # the 2 x 2 interior of each box finds no ground: its lowest voxels pass for it
    wide = cref.columns(r, ground_radius=3, thickness=1)                             # the minimum filter undershoots a slope by slope x R
    assert _capability_errors(wide, label, rows) > 0 == _capability_errors(cref.columns(r, ground_radius=3, thickness=2), label, rows)
    z = np.array([c[2] for c, _ in rows])
    truth = np.array([label[c] == 'ramp' for c, _ in rows])
    errors = [int(((z <= t) != truth).sum()) for t in range(int(z.min()) - 1, int(z.max()) + 1)]
    assert min(errors) == 320                                                        # the best single threshold


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_columns_workspace_bytes', 'pcacc_accum_columns', 'pcacc_accum_bev'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C17. ' in header and len(native._PROTOTYPES['pcacc_accum_columns']) == 36 and len(native._PROTOTYPES['pcacc_accum_bev']) == 25
    assert len(native._PROTOTYPES['pcacc_accum_columns_workspace_bytes']) == 2
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = open(os.path.join(csrc, 'accum_columns.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_normals.h"']
    for helper in ('accum_unkey(', 'accum_lower_bound(', 'accum_field(', 'accum_centroid(', 'accn_centroid(', 'accn_index(', 'accn_in_range(', 'PCACC_BOUND(',
                   'PCACC_NO_CONTRACT'):
        assert helper in text, helper
    kernels = open(os.path.join(csrc, 'accum_columns.hip')).read()
    assert 'accn_rows_launch(' in kernels and 'pcacc_scan_i32(' in kernels and 'accum_wave_count(' in kernels and 'asm' not in kernels
    assert 'atomicAdd' not in kernels and '__shared__' not in kernels
    assert 'accum_columns.hip' in open(os.path.join(csrc, 'Makefile')).read()
    for name, value in (('COLUMNS_MAX_RADIUS', 8), ('COLUMNS_MAX_HEIGHT', 2097151), ('COLUMNS_COUNTERS', 5), ('COLUMNS_N_ROWS', 0), ('COLUMNS_N_COLUMNS', 1),
                        ('COLUMNS_N_GROUND', 2), ('COLUMNS_N_BAND', 3), ('COLUMNS_N_BORROWED', 4)):
        assert ('#define PCACC_%s %d\n' % (name, value)) in header and getattr(native, name) == value
    assert native.BEV_MAX_PIXELS == cref.MAX_PIXELS == 1 << 28 and (cref.MAX_RADIUS, cref.MAX_HEIGHT) == (8, 2097151)
    assert [f for f, _, _ in native.COLUMN_FIELDS] == ['key'] + list(cref.COLUMN_FIELDS) and [f for f, _, _ in native.COLUMN_ROW_FIELDS] == list(cref.ROW_FIELDS)
    assert [f for f, _, _ in native.BEV_FIELDS] == list(cref.BEV_FIELDS)
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    for call in (cpu.columns, cpu.ground_mask, cpu.split_ground, cpu.bev):
        with pytest.raises(native.NativeError):
            call()
        for bad in BAD_COLUMN_ARGS:
            with pytest.raises(ValueError):                                          # before anything is allocated: a CPU map gets this far
                call(**bad)
    for bad in BAD_WINDOWS:
        with pytest.raises(ValueError):
            cpu.bev(**bad)


BAD_COLUMN_ARGS = (dict(ground_radius=-1), dict(ground_radius=9), dict(thickness=-1), dict(thickness=1 << 21), dict(band=(-1, 3)), dict(band=(4, 3)),
                   dict(band=(0, 1 << 21)), dict(band=(1, 2, 3)), dict(band=None), dict(min_count=0), dict(max_moving_fraction=float('nan')))
BAD_WINDOWS = (dict(origin=(0, 0), shape=(0, 4)), dict(origin=(0, 0), shape=(4, 0)), dict(origin=(0, 0), shape=(1 << 14, (1 << 14) + 1)),
               dict(origin=(0, 0, 0), shape=(2, 2)), dict(origin=((1 << 31) + 1, 0), shape=(2, 2)), dict(origin=(0, 0), shape=(2, 2, 2)))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
_clouds = {}


def _cloud(scene):
    """A device map per scene, shared: the calls do not modify it (a test below says so)."""
    if scene not in _clouds:
        _clouds[scene] = ah.device_cloud(_scene(scene))
    return _clouds[scene]


def _poisoned(fields, lead):
    """Every byte of every output 0xa5 (accum_host.h's POISON_BYTE), whatever its type."""
    return {name: torch.full((int(np.prod(lead + shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size(),), 0xa5, dtype=torch.uint8, device=DEV)
            .view(dtype).reshape(lead + shape) for name, dtype, shape in fields}


def _is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == 0xa5).all())


def _binding(m, args, windows):
    """One call of each binding with every output and the counts poisoned first.  -> the tables sliced to their counts, and the images."""
    from pcaccumulation_amd import native
    a = dict(args)
    R, thickness, lo, hi, min_count = m._column_args(a.pop('ground_radius'), a.pop('thickness'), a.pop('band'), a.get('min_count', 1), a.get('max_moving_fraction'))
    f = (min_count, a.get('max_moving_fraction'))
    m._ensure()
    rows = m.num_voxels
    out = _poisoned(native.COLUMN_FIELDS + native.COLUMN_ROW_FIELDS, (rows,))
    counters = torch.full((5,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    n = torch.full((2,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    res = native.accum_columns(m._cur, rows, *f, R, thickness, lo, hi, out=out, counters=counters, n=n)
    kept, C = res.pop('n').tolist()
    for name, _, _ in native.COLUMN_FIELDS:                                          # the rows behind the ones in use keep their poison
        assert _is_poison(res[name][C:]), name
    for name, _, _ in native.COLUMN_ROW_FIELDS:
        assert _is_poison(res[name][kept:]), name
    res = {name: (t if name == 'counters' else t[:kept] if name.startswith('row_') else t[:C]) for name, t in res.items()}
    images = []
    for (x0, y0), (H, W) in windows:
        image = native.accum_bev(m._cur, rows, *f, res, x0, y0, W, H, out=_poisoned(native.BEV_FIELDS, (H, W)))
        images.append(image)
    return dict(res, kept=kept, n_columns=C), images


def _numpy(res):
    return {name: (t.tolist() if name == 'counters' else t.cpu().numpy() if torch.is_tensor(t) else t) for name, t in res.items()}


def _same_bits(a, b):
    return all(torch.equal(a[f].view(torch.int64) if a[f].dtype == torch.float64 else a[f].view(torch.int32) if a[f].dtype == torch.float32 else a[f],
                           b[f].view(torch.int64) if b[f].dtype == torch.float64 else b[f].view(torch.int32) if b[f].dtype == torch.float32 else b[f])
               for f in a if torch.is_tensor(a[f]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernels_equal_the_host_build_gpu(host_exe, tmp_path, name):
    scene, args = CASES[name]
    host, windows = _host(host_exe, tmp_path, name), _windows(name)
    m = _cloud(scene)
    snap = ah.snapshot(m, whole_sidecar=True)
    res, images = _binding(m, args, windows)
    assert (res['kept'], res['n_columns']) == (host['kept'], host['n_columns'])
    assert all(t.is_cuda for t in res.values() if torch.is_tensor(t)) and res['counters'].dtype == torch.int64
    _assert_same(_numpy(res), host, name, ('key',) + cref.COLUMN_FIELDS + cref.ROW_FIELDS)
    for w, image, want in zip(windows, images, host['images']):
        _assert_same_image(_numpy(image), want, (name, w))
    again, images_again = _binding(m, args, windows)                                 # a second run gives the same bits
    assert _same_bits(res, again) and all(_same_bits(a, b) for a, b in zip(images, images_again))
    method = m.columns(**args)                                                       # the methods: the same calls
    _assert_same(_numpy(method), host, name + ' (method)', ('key',) + cref.COLUMN_FIELDS + cref.ROW_FIELDS)
    f = {a: args[a] for a in ('min_count', 'max_moving_fraction') if a in args}
    assert np.array_equal(m.ground_mask(**args).cpu().numpy(), host['row_is_ground'] != 0)
    assert method['row_column'].shape[0] == m.extract(**f)['points'].shape[0]
    for (origin, shape), want in list(zip(windows, host['images']))[:4]:
        got = m.bev(origin, shape, **args)
        _assert_same_image(_numpy({k: got[k] for k in cref.BEV_FIELDS}), want, (name, origin, shape, 'method'))
        assert got['origin'] == origin and got['voxel_size'] == m.voxel_size and _same_bits(got['columns'], method)
    if scene != 'edge':
        box = m.bev(**args)                                                          # None: the bounding box of the columns
        origin, shape = cref.bounding_box(_restate(name))
        assert box['origin'] == origin and tuple(box['column'].shape) == shape
        _assert_same_image(_numpy({k: box[k] for k in cref.BEV_FIELDS}), cref.bev(_restate(name), origin, shape), (name, 'box'))
    else:
        with pytest.raises(ValueError):                                              # 2^21 x 2^21 columns
            m.bev(**args)
    ah.assert_unchanged(m, snap, name)                                               # read-only: keys, records, stamps, state words, num_voxels


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['dense11_r2', 'rows343_r2_filtered', 'tower_r1', 'flat300_r8_filtered', 'capability_r2'])
def test_tables_agree_with_extract_and_records_gpu(name):
    scene, args = CASES[name]
    m = _cloud(scene)
    f = {a: args[a] for a in ('min_count', 'max_moving_fraction') if a in args}
    e, cols = _numpy(m.extract(**f)), _numpy(m.columns(**args))
    C, V = cols['xy'].shape[0], e['coords'].shape[0]
    assert C > 0 and cols['row_column'].shape == (V,) and cols['counters'][:2] == [V, C]
    for c in range(C):                                                               # the run of every column in extract(): its xy, z_low / z_high at the ends
        run = e['coords'][cols['first_row'][c]:cols['first_row'][c] + cols['voxels'][c]]
        assert (run[:, :2] == cols['xy'][c]).all() and run[0, 2] == cols['z_low'][c] and run[-1, 2] == cols['z_high'][c] and (np.diff(run[:, 2]) > 0).all()
    assert int(cols['points'].sum()) == int(e['count'].sum()) and int(cols['moving'].sum()) == int(e['moving'].sum())
    assert np.array_equal(np.repeat(np.arange(C), cols['voxels']), cols['row_column'])
    assert np.array_equal(e['coords'][:, 2] - cols['ground_z'][cols['row_column']], cols['row_height'])
    box = _numpy({k: v for k, v in m.bev(**args).items() if k in cref.BEV_FIELDS})
    at = box['column'] >= 0
    top = cols['first_row'] + cols['voxels'] - 1
    assert at.sum() == C and np.array_equal(ah.bits(box['elevation'][at]), ah.bits(e['points'][top[box['column'][at]], 2]))
    assert np.array_equal(ah.bits(box['ground'][at]), ah.bits(e['points'][cols['ground_row'][box['column'][at]], 2]))
    keys, acc, _ = m.records()                                                       # row_height_m again, in numpy float64 from the records
    acc = acc.reshape(5, -1)
    keep = np.array([rref.keep(int(c), int(mv), f.get('min_count', 1), f.get('max_moving_fraction')) for c, mv in zip(acc[0], acc[1])])
    z = (acc[4, keep].astype(np.float64) / acc[0, keep].astype(np.float64)) * (1.0 / 65536.0)
    assert np.array_equal(ah.bits(z - z[cols['ground_row'][cols['row_column']]]), ah.bits(cols['row_height_m']))


@pytest.mark.gpu
def test_split_ground_gpu():
    """The capability scene: the ground map is the ramp, the rest is boxes and canopy, and the two merge back into the original records bit for bit."""
    r = _scene('capability')
    _, label = _capability()
    m = ah.device_cloud(r)
    snap = ah.snapshot(m, whole_sidecar=True)
    ground, rest = m.split_ground(ground_radius=2, thickness=1)
    assert ground.num_voxels == 1552 and rest.num_voxels == 676
    assert {tuple(c) for c in ground.extract()['coords'].tolist()} == {c for c, v in label.items() if v == 'ramp'}
    assert {tuple(c) for c in rest.extract()['coords'].tolist()} == {c for c, v in label.items() if v != 'ramp'}
    ah.assert_unchanged(m, snap, 'split_ground')
    whole = ground.copy()
    whole.merge(rest)
    assert whole.num_voxels == m.num_voxels and all(np.array_equal(a, b) for a, b in zip(whole.records(), m.records()))
    band = m.columns(ground_radius=2, thickness=1, band=(2, 20))
    assert band['counters'].tolist() == [2228, 1600, 1552, 576, band['counters'].tolist()[4]]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['rows343_r2', 'flat300_r1', 'capability_r2'])
def test_bev_is_the_scatter_of_columns_gpu(name):
    scene, args = CASES[name]
    m = _cloud(scene)
    cols, e = _numpy(m.columns(**args)), _numpy(m.extract())
    (x0, y0), (H, W) = cref.bounding_box(_restate(name))
    for origin, shape in (((x0, y0), (H, W)), ((x0 + 2, y0 - 3), (H + 1, max(W - 1, 1)))):
        want = dict(column=np.full(shape, -1, np.int32), elevation=np.full(shape, np.nan, np.float32), ground=np.full(shape, np.nan, np.float32),
                    band_top=np.full(shape, -1, np.int32), voxels=np.zeros(shape, np.int32))
        r, c = cols['xy'][:, 1] - origin[1], cols['xy'][:, 0] - origin[0]
        at = (r >= 0) & (r < shape[0]) & (c >= 0) & (c < shape[1])
        want['column'][r[at], c[at]] = np.flatnonzero(at)
        want['elevation'][r[at], c[at]] = e['points'][(cols['first_row'] + cols['voxels'] - 1)[at], 2]
        want['ground'][r[at], c[at]] = e['points'][cols['ground_row'][at], 2]
        want['band_top'][r[at], c[at]], want['voxels'][r[at], c[at]] = cols['band_top'][at], cols['voxels'][at]
        got = m.bev(origin, shape, **args)
        _assert_same_image(_numpy({k: got[k] for k in cref.BEV_FIELDS}), want, (name, origin))


def _assert_equals_restatement(m, r, what, **args):
    want = cref.columns(r, **args)
    got = _numpy(m.columns(**args))
    _assert_same(got, want, what)
    origin, shape = cref.bounding_box(want)
    box = m.bev(**args)
    assert box['origin'] == origin
    _assert_same_image(_numpy({k: box[k] for k in cref.BEV_FIELDS}), cref.bev(want, origin, shape), what)
    return got


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1)
    floor = ah.centres([(x, y, (x + y) // 3) for x in range(4, 10) for y in range(-3, 3)], 0.1)
    post = ah.centres([(6, 0, z) for z in range(4, 12)] + [(7, -1, z) for z in (5, 6)], 0.1)

    def both_add(pts, stamp):
        m.add(torch.from_numpy(pts).to(DEV), None, stamp=stamp)
        r.add(pts, None, stamp=stamp)
    both_add(np.concatenate([floor, floor[::2], post]), 0)
    a = _assert_equals_restatement(m, r, 'after add', ground_radius=1, thickness=1, band=(2, 20), min_count=2)
    both_add(np.concatenate([floor[::3], ah.centres([(9, 1, 14), (6, 0, 20)], 0.1)]), 3)
    assert m.prune(before_stamp=2)['kept'] == rref.prune(r, None, before_stamp=2)[0] > 0      # what stamp 3 did not touch goes
    b = _assert_equals_restatement(m, r, 'after prune', ground_radius=2, thickness=0, band=(1, 30))
    assert b['counters'] != a['counters']
    both_add(ah.centres([(-9, 0, 0), (6, 0, 0), (6, 0, 1), (6, 9, 9)], 0.1), 4)
    c = _assert_equals_restatement(m, r, 'add after prune', ground_radius=8, thickness=2, band=(2, 20))
    path = os.path.join(str(tmp_path), 'map.npz')
    m.save(path)
    d = _assert_equals_restatement(AccumulatedCloud.load(path, DEV), r, 'after load', ground_radius=8, thickness=2, band=(2, 20))
    assert all(np.array_equal(ah.bits(c[f]), ah.bits(d[f])) for f in cref.COLUMN_FIELDS + cref.ROW_FIELDS) and c['counters'] == d['counters']


@pytest.mark.gpu
def test_columns_on_the_model_forward_gpu(golden):
    """add_results on the model_tiny_test forward, then columns() and bev(): they run and the counters are consistent.  Nothing more is claimed."""
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
    cols = m.columns(ground_radius=2, thickness=1, band=(2, 20))
    V, C = m.extract()['points'].shape[0], cols['xy'].shape[0]
    assert V == m.num_voxels > 0 and cols['row_height'].shape == (V,) and int(cols['voxels'].sum()) == V
    assert cols['counters'].tolist() == [V, C, int(cols['row_is_ground'].sum()), int(cols['band_voxels'].sum()),
                                         int((cols['ground_column'] != torch.arange(C, device=dev)).sum())]
    image = m.bev(ground_radius=2, thickness=1, band=(2, 20))
    assert int((image['column'] >= 0).sum()) == C and int(image['voxels'].sum()) == V
    assert bool(torch.isnan(image['elevation']).eq(image['column'] < 0).all())


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    m = ah.device_cloud(_scene('rows65'))
    snap = ah.snapshot(m, whole_sidecar=True)
    fields = native.COLUMN_FIELDS + native.COLUMN_ROW_FIELDS
    out = {name: torch.full((65,) + shape, 7, dtype=dtype, device=DEV) for name, dtype, shape in fields}
    image = {name: torch.full((4, 6), 7, dtype=dtype, device=DEV) for name, dtype, _ in native.BEV_FIELDS}
    counters, n = torch.full((5,), 7, dtype=torch.int64, device=DEV), torch.full((2,), 7, dtype=torch.int64, device=DEV)
    good = dict(tables=m._cur, m=65, min_count=1, max_moving_fraction=None, ground_radius=2, thickness=1, band_lo=2, band_hi=20, out=out, counters=counters, n=n)
    for bad in (dict(ground_radius=-1), dict(ground_radius=9), dict(thickness=-1), dict(thickness=1 << 21),
                dict(band_lo=-1), dict(band_lo=21), dict(band_hi=1 << 21)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_columns(**dict(good, **bad))
    real = m.columns()                                                               # column tables to hand to the raster
    lib = native.lib()
    keys, acc, stamps = (native._dev(t) for t in m._cur)
    ptr = [native._dev(out[name]) for name, _, _ in fields]
    iptr = [native._dev(image[name]) for name, _, _ in native.BEV_FIELDS]
    cptr = [native._dev(real[name]) for name in ('key', 'first_row', 'voxels', 'ground_row', 'band_top')]
    C = real['key'].shape[0]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def call(ptr=ptr, keys=keys, acc=acc, stamps=stamps, out_n=native._dev(n), cnt=native._dev(counters), ws=native._dev(ws), ws_bytes=ws.numel(), rows=65,
             cap=m.capacity, R=2, thickness=1, lo=2, hi=20):
        return lib.pcacc_accum_columns(keys, acc, stamps, cap, rows, 1, 0, 0.0, R, thickness, lo, hi, *ptr, out_n, cnt, ws, ws_bytes, native._stream())

    def raster(iptr=iptr, cptr=cptr, keys=keys, acc=acc, ws=native._dev(ws), ws_bytes=ws.numel(), rows=65, cap=m.capacity, n_col=C, x0=-3, y0=-3, W=6, H=4):
        return lib.pcacc_accum_bev(keys, acc, cap, rows, 1, 0, 0.0, *cptr, n_col, x0, y0, W, H, *iptr, ws, ws_bytes, native._stream())
    assert call(rows=-1) == call(rows=m.capacity + 1) == call(cap=(1 << 30) + 1) == call(R=-1) == call(R=9) == call(thickness=-1) == call(thickness=1 << 21) == -1
    assert call(lo=-1) == call(lo=21) == call(hi=1 << 21) == -1
    assert call(keys=None) == call(acc=None) == call(stamps=None) == call(out_n=None) == call(cnt=None) == call(ws=None) == call(ws_bytes=16) == -1
    for j in range(len(ptr)):
        assert call(ptr=ptr[:j] + [None] + ptr[j + 1:]) == -1, j                     # a NULL output of non-zero size
    inside = [native.ctypes.c_void_p(m._cur[0].data_ptr() + 8), native.ctypes.c_void_p(m._cur[1].data_ptr() + 8 * m.capacity),
              native.ctypes.c_void_p(m._cur[2].data_ptr() + 4 * m.capacity)]
    for j in (0, 2, 17, 18):                                                         # an output that shares bytes with the keys, the records, the stamps
        for p in inside:
            assert call(ptr=ptr[:j] + [p] + ptr[j + 1:]) == -1, j
    assert call(out_n=inside[1]) == call(cnt=inside[0]) == -1
    assert raster(rows=-1) == raster(rows=m.capacity + 1) == raster(n_col=-1) == raster(n_col=66) == raster(W=0) == raster(H=0) == raster(W=-1) == -1
    assert raster(W=1 << 14, H=(1 << 14) + 1) == raster(W=(1 << 28) + 1, H=1) == raster(W=1 << 40, H=1 << 40) == -1
    assert raster(x0=(1 << 31) + 1) == raster(y0=-(1 << 31) - 1) == raster(keys=None) == raster(acc=None) == raster(ws=None) == raster(ws_bytes=16) == -1
    for j in range(5):
        assert raster(iptr=iptr[:j] + [None] + iptr[j + 1:]) == raster(cptr=cptr[:j] + [None] + cptr[j + 1:]) == -1, j
        assert raster(iptr=iptr[:j] + [inside[0]] + iptr[j + 1:]) == raster(iptr=iptr[:j] + [inside[1]] + iptr[j + 1:]) == -1, j
    need = native.ctypes.c_size_t(0)
    assert lib.pcacc_accum_columns_workspace_bytes(-1, native.ctypes.byref(need)) == lib.pcacc_accum_columns_workspace_bytes(65, None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in list(out.values()) + list(image.values()) + [counters, n])       # nothing was launched: the poison stands
    ah.assert_unchanged(m, snap, 'bad arguments')
    for call_ in (m.columns, m.ground_mask, m.split_ground, m.bev):
        for bad in BAD_COLUMN_ARGS:
            with pytest.raises(ValueError):
                call_(**bad)
    for bad in BAD_WINDOWS:
        with pytest.raises(ValueError):
            m.bev(**bad)
    assert call() == 0 and n.tolist() == [65, C] and counters.tolist()[:2] == [65, C] and not bool((out['row_is_ground'] == 7).any())
    assert raster() == 0 and not bool((image['voxels'] == 7).any()) and int((image['column'] >= 0).sum()) > 0
    assert raster(n_col=0, cptr=[None] * 5) == 0 and bool((image['column'] == -1).all()) and bool(torch.isnan(image['ground']).all())     # C = 0: all empty
    empty = native.accum_columns(**dict(good, m=0, out={f: t[:0] for f, t in out.items()}))       # m = 0: zero counts and nothing else
    assert empty['counters'].tolist() == [0] * 5 and empty['n'].tolist() == [0, 0]
    ah.assert_unchanged(m, snap, 'after all')
