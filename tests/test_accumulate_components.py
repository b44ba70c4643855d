"""Connected components of the accumulated scene cloud (include/pcacc.h C11): AccumulatedCloud.components / remove_components.

A label is a pure function of the map (a component is numbered by the position of its smallest key), so every claim is an equality of integers or of
float32 bits:
  CPU   the g++ build of csrc/accum_components.h and union_find.h (tests/accum_components_host_driver.cpp, every table index asserted, the joins in a
        scrambled order, poison behind the rows in use) against the plain-Python flood fill on a coordinate set
        (tests/accumulate_components_reference.py): labels, every per-component table, counters, surviving keys, records, stamps, ray counts;
  GPU   the kernels against the g++ build on the same scenes, identities that tie the tables to extract(), the blob scene that prune() cannot clean,
        objects on a ground sheet, a life cycle against the restatement, the model forward and the argument checks."""
import os

import numpy as np
import pytest
import torch

import accumulate_components_reference as cref
import accumulate_helpers as ah
import accumulate_prune_reference as rref
import accumulate_reference as ref
import test_accumulate_prune as tp
from accumulate_helpers import DEV
from helpers import ROOT
TABLES = (('voxels', np.int32, ()), ('points', np.int64, ()), ('moving', np.int64, ()), ('sum_q', np.int64, (3,)), ('centroid', np.float32, (3,)),
          ('lo', np.int32, (3,)), ('hi', np.int32, (3,)), ('t_first', np.int32, ()), ('t_last', np.int32, ()), ('first_row', np.int32, ()))
FILTER = dict(min_count=2, max_moving_fraction=0.5)


# ---- scenes: a ReferenceMap and a {coord: rays} dict (None: no sidecar), built once and never modified ----------------------------------------
def _serpentine():
    """A 33 x 33 path in the plane z = 0: full columns at even x, joined at y = 32 and y = 0 in turn -- one component whose walk runs with and against
    the key order."""
    path = [(x, y, 0) for x in range(0, 33, 2) for y in range(33)]
    return path + [(x, 32 if (x // 2) % 2 == 0 else 0, 0) for x in range(1, 33, 2)]


def _blob_scene():
    """The sheet of section 9g's noisy plane (3 m x 3 m, 1 cm noise, no strays) and five floating 3 x 3 x 3 blobs: every blob voxel has at least 8
    voxels within one voxel of it, itself included."""
    rs = np.random.RandomState(21)
    sheet = np.concatenate([rs.uniform(-1.5, 1.5, (6000, 2)), rs.normal(0.02, 0.01, (6000, 1))], 1).astype(np.float32)
    blobs = [(x0 + a, y0 + b, z0 + c) for x0, y0, z0 in ((-12, -12, 6), (-3, 8, 9), (5, -9, 12), (10, 10, 7), (0, 0, 15))
             for a in range(3) for b in range(3) for c in range(3)]
    return sheet, blobs


def _wavy_blobs():
    """The 76 661-voxel sheet of section 9d and forty stray 2 x 2 x 2 blobs above it: 76 981 voxels, m mod 64 != 0 and m mod 256 != 0."""
    rs = np.random.RandomState(5)
    corners = {(int(x), int(y), int(z)) for x, y, z in zip(rs.randint(-60, 60, 40) * 2, rs.randint(-60, 60, 40) * 2, rs.randint(12, 30, 40))}
    blobs = [(x + a, y + b, z + c) for x, y, z in sorted(corners) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    return np.concatenate([ah.wavy(), ah.centres(blobs, 0.1)]).astype(np.float32)


def _sizes_scene():
    """Components of 1 .. 5 voxels in a row along y (spaced 10 apart in x), every voxel 3 points, so that points = 3 voxels; a voxel of count 1 next to
    each (outside FILTER's min_count = 2, and a bridge to nothing); ray counts on all of them."""
    rows, pierced = {}, {}
    for n in range(1, 6):
        for k in range(n):
            rows[(10 * n, k, 0)] = (3, 0, n, n + k)
            pierced[(10 * n, k, 0)] = n + k
        rows[(10 * n, n, 0)] = (1, 0, 0, 9)
        pierced[(10 * n, n, 0)] = 50 + n
    return ah.records(0.1, rows), pierced


def _build_scene(name):
    one = (1, 0, 0, 0)
    if name.startswith('rows') or name in ('ratio', 'bound', 'wavy'):
        return tp._scene(name)
    if name == 'chain_x':
        return ah.records(0.1, {(k - 500, 3, -2): (1, 0, k % 7, k % 7 + 1) for k in range(1025)}), None
    if name == 'chain_z':
        return ah.records(0.1, {(3, -2, k - 500): (2, 1, 0, k % 5) for k in range(1025)}), None
    if name == 'serpentine':
        return ah.records(0.1, {c: one for c in _serpentine()}), None
    if name == 'corners':
        return ah.records(0.1, {c: one for c in [(k, k, k) for k in range(8)] + [(-k, k, -k) for k in range(1, 8)]}), None
    if name == 'lattice2':
        return ah.records(0.1, {(2 * a, 2 * b, 2 * c): one for a in range(4) for b in range(4) for c in range(4)}), None
    if name == 'lattice4':
        return ah.records(0.1, {(4 * a, 4 * b, 4 * c): one for a in range(3) for b in range(3) for c in range(3)}), None
    if name == 'walls':
        return ah.records(0.1, {(x, y, z): one for x in (0, 2) for y in range(5) for z in range(5)}), None
    if name == 'dumbbell':
        rows = {(x0 + a, b, c): (3, 0, 0, 0) for x0 in (0, 4) for a in range(3) for b in range(3) for c in range(3)}
        rows[(3, 1, 1)] = one                                                        # the bridge
        return ah.records(0.1, rows), None
    if name == 'sizes':
        return _sizes_scene()
    if name == 'blobs':
        sheet, blobs = _blob_scene()
        return ah.points_map(0.1, [(np.concatenate([sheet, ah.centres(blobs, 0.1)]), None, 0)]), None
    assert name == 'wavy_blobs'
    return ah.points_map(0.1, [(_wavy_blobs(), None, 0)]), None


_scenes = {}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _build_scene(name)
    return _scenes[name]


def _filter(args):
    return dict(min_count=args.get('min_count', 1), max_moving_fraction=args.get('max_moving_fraction'))


def _mask(scene, args):
    """The mask of a case as a uint8 array over extract's rows, or None: ('random', seed), ('without', coords) or ('rows', n) -- all ones, n entries."""
    spec = args.get('mask')
    if spec is None:
        return None
    kept = cref.kept_coords(_scene(scene)[0], **_filter(args))
    if spec[0] == 'random':
        return (np.random.RandomState(spec[1]).rand(len(kept)) < 0.7).astype(np.uint8)
    if spec[0] == 'without':
        return np.array([0 if c in spec[1] else 1 for c in kept], np.uint8)
    return np.ones(len(kept) + spec[1], np.uint8)


# ---- cases: a scene and the arguments of components() + remove_components() ----------------------------------------------------------------------
def _cases():
    cases = {}
    for m in tp.ROW_COUNTS:
        for r in (1, 2, 3):
            cases['rows%d_r%d' % (m, r)] = ('rows%d' % m, dict(radius=r))
            cases['rows%d_r%d_filter_mask' % (m, r)] = ('rows%d' % m, dict(radius=r, mask=('random', 10 * m + r), min_voxels=3, **FILTER))
    cases['rows_no_sidecar'] = ('rows_no_sidecar', dict(radius=1, min_voxels=2))
    for scene in ('chain_x', 'chain_z', 'serpentine', 'corners'):
        cases[scene] = (scene, dict(radius=1))
    for scene, radii in (('lattice2', (1, 2)), ('lattice4', (3,)), ('walls', (1, 2)), ('bound', (1, 2, 3))):
        for r in radii:
            cases['%s_r%d' % (scene, r)] = (scene, dict(radius=r))
    cases['dumbbell'] = ('dumbbell', dict(radius=1))
    cases['dumbbell_min_count'] = ('dumbbell', dict(radius=1, min_count=2))
    cases['dumbbell_mask'] = ('dumbbell', dict(radius=1, mask=('without', {(3, 1, 1)})))
    for k, (f, _) in enumerate(tp.RATIO_FILTERS):
        cases['ratio_filter%d' % k] = ('ratio', dict(radius=3, **f))
    cases['mask_too_long'] = ('rows65', dict(radius=1, mask=('rows', 1), min_voxels=3))
    cases['mask_too_short'] = ('rows65', dict(radius=2, mask=('rows', -1), **FILTER))
    cases['mask_all_ones'] = ('rows65', dict(radius=1, mask=('rows', 0)))
    for tag, a in (('voxels3', dict(min_voxels=3)), ('voxels4', dict(min_voxels=4)), ('points9', dict(min_points=9)), ('points10', dict(min_points=10)),
                   ('both', dict(min_voxels=2, min_points=12)), ('everything', dict(min_voxels=100)), ('nothing', dict(min_voxels=1, min_points=1)),
                   ('dry_run', dict(min_voxels=4, dry_run=True))):
        cases['sizes_' + tag] = ('sizes', dict(radius=1, min_count=2, **a))
    cases['sizes_mask'] = ('sizes', dict(radius=1, min_count=2, min_voxels=4, mask=('without', {(50, 0, 0), (40, 1, 0)})))
    cases['blobs'] = ('blobs', dict(radius=1, min_voxels=100))
    return cases


CASES = _cases()
CASE_NAMES = sorted(CASES)
BIG = {'wavy_r1': dict(radius=1, min_voxels=9), 'wavy_r2': dict(radius=2, min_points=40), 'wavy_mask': dict(radius=1, mask=('random', 3), min_voxels=20)}

_restated = {}


def _restate(name):
    """The restatement's result of a case, computed once: components, remove counters, surviving records and ray counts in key order."""
    if name not in _restated:
        scene, args = CASES[name]
        r, pierced = tp._copy(*_scene(scene))
        mask = _mask(scene, args)
        a = dict(radius=args['radius'], mask=None if mask is None else mask.tolist(), **_filter(args))
        comp = cref.components(r, **a)
        removed = cref.remove_components(r, pierced, args.get('min_voxels', 0), args.get('min_points', 0), args.get('dry_run', False), **a)
        keys, acc, stamps = r.records()
        _restated[name] = dict(comp, remove_counters=removed, keys=keys, acc=acc.reshape(5, -1), stamps=stamps.reshape(2, -1),
                               pierced=None if pierced is None else ah.aligned(pierced, keys))
    return _restated[name]


# ---- the host build -------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_components_host_driver', 'components_host')


def _run_host(exe, tmp_path, tag, records, pierced, mask, spare_in=3, spare_out=5, radius=1, min_count=1, max_moving_fraction=None, min_voxels=0, min_points=0,
              dry_run=False, seed=1):
    m = records[0].shape[0]
    head = [m, max(m + spare_in, 1), max(m + spare_out, 1), 0 if pierced is None else 1, 0 if mask is None else 1, 0 if mask is None else len(mask), min_count,
            0 if max_moving_fraction is None else 1, radius, min_voxels, min_points, 1 if dry_run else 0, seed]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array([0.0 if max_moving_fraction is None else max_moving_fraction], np.float64),
                        ah.map_bytes(*records, pierced), b'' if mask is None else np.ascontiguousarray(mask, np.uint8))
    head = np.frombuffer(raw, np.int64, 12)
    out = dict(counters=head[:7].tolist(), remove_counters=head[7:11].tolist(), edges=int(head[11]))
    kept, k = out['counters'][0] - out['counters'][2], out['counters'][4]
    fields = [('label', np.int32, (kept,))] + [(n, d, (k,) + s) for n, d, s in TABLES]
    if not dry_run and out['counters'][6] == cref.OK:
        fields += ah.map_layout(out['remove_counters'][0], pierced is not None)
    tables, off = ah.unpack(raw, 96, fields)
    assert off == len(raw)
    out.update(tables)
    if pierced is None:
        out['pierced'] = None
    return out


def _host_args(args):
    return {k: v for k, v in args.items() if k != 'mask'}


_hosted = {}


def _host(exe, tmp_path, name):
    if name not in _hosted:
        scene, args = CASES[name] if name in CASES else ('wavy_blobs', BIG[name])
        r, pierced = _scene(scene)
        keys = r.records()[0]
        _hosted[name] = _run_host(exe, tmp_path, name, r.records(), None if pierced is None else ah.aligned(pierced, keys), _mask(scene, args),
                                  **_host_args(args))
    return _hosted[name]


def _assert_components_equal(got, want, what):
    """got: arrays; want: arrays or the restatement's lists.  Floats also as their integer views."""
    assert list(got['counters']) == list(want['counters']), what
    assert np.array_equal(got['label'], np.asarray(want['label'], np.int32).reshape(-1)), what
    for name, dtype, shape in TABLES:
        w = np.asarray(want[name], dtype).reshape((-1,) + shape)
        assert got[name].dtype == dtype and got[name].shape == w.shape and np.array_equal(got[name], w), (what, name)
    assert np.array_equal(got['centroid'].view(np.int32), np.asarray(want['centroid'], np.float32).reshape(-1, 3).view(np.int32)), what


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for():
    count = lambda name: _restate(name)['counters'][4]
    assert [_scene('rows%d' % m)[0].num_voxels for m in tp.ROW_COUNTS] == list(tp.ROW_COUNTS)
    assert _scene('chain_x')[0].num_voxels == _scene('chain_z')[0].num_voxels == 1025 and count('chain_x') == count('chain_z') == 1
    keys = _scene('chain_z')[0].records()[0]
    assert np.array_equal(np.diff(keys), np.ones(1024, np.int64))                 # contiguous rows: four workgroups of 256 on one component
    assert _scene('serpentine')[0].num_voxels == 17 * 33 + 16 and count('serpentine') == 1
    assert count('corners') == 1 and _restate('corners')['voxels'] == [15]
    assert (count('lattice2_r1'), count('lattice2_r2'), count('lattice4_r3')) == (64, 1, 27)
    assert (count('walls_r1'), count('walls_r2')) == (2, 1)
    assert (count('dumbbell'), count('dumbbell_min_count'), count('dumbbell_mask')) == (1, 2, 2)
    assert _restate('dumbbell_mask')['counters'][:4] == [55, 54, 0, 1] and _restate('dumbbell_min_count')['counters'][:4] == [55, 54, 1, 0]
    for k, (_, kept) in enumerate(tp.RATIO_FILTERS):
        c = _restate('ratio_filter%d' % k)['counters']
        assert c[1] == kept and c[0] == 7 and c[2] == 7 - kept, k
    for name in ('mask_too_long', 'mask_too_short'):
        res = _restate(name)
        assert res['counters'][4:] == [0, 0, cref.BAD_MASK] and set(res['label']) == {-1} and res['remove_counters'] == [65, 0, 0, 0], name
    assert _restate('mask_all_ones')['label'] == _restate('rows65_r1')['label']
    assert _scene('wavy_blobs')[0].num_voxels == 76661 + 320 and 76981 % 64 != 0 and 76981 % 256 != 0


def test_no_link_through_an_overflowed_field():
    """The index-bound scene at 0.01 m with its decoys: the components are those of a direct Chebyshev flood fill on the coordinates."""
    vox, decoys = ah.bound_voxels()
    cells = set(vox + decoys)
    for r in (1, 2, 3):
        todo, n = set(cells), 0
        while todo:
            grow = [todo.pop()]
            while grow:
                c = grow.pop()
                near = [v for v in todo if max(abs(a - b) for a, b in zip(c, v)) <= r]
                todo.difference_update(near)
                grow.extend(near)
            n += 1
        assert _restate('bound_r%d' % r)['counters'][4] == n and n >= 6, r


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    host, want = _host(host_exe, tmp_path, name), _restate(name)
    _assert_components_equal(host, want, name)
    assert host['remove_counters'] == want['remove_counters'], name
    assert host['counters'][0] == host['counters'][1] + host['counters'][2] + host['counters'][3], name
    if 'keys' in host:
        tp._assert_same(dict(host, counters=[]), dict(want, counters=[]), name)
    scene, args = CASES[name]
    r, pierced = _scene(scene)
    other = _run_host(host_exe, tmp_path, name + '_seed', r.records(), None if pierced is None else ah.aligned(pierced, r.records()[0]), _mask(scene, args),
                      spare_in=0, spare_out=0, seed=12345, **_host_args(args))   # another order of the joins, tables with no spare row
    assert all(np.array_equal(other[f], host[f]) for f in host if host[f] is not None), name


def test_removal_thresholds_on_the_restatement():
    """voxels == min_voxels stays and one less goes; the same for points; rows outside the filter or the mask survive with their records and ray counts."""
    kept_sizes = lambda name: _restate(name)['remove_counters']
    assert kept_sizes('sizes_voxels3') == [5 + 3 + 4 + 5, 1 + 2, 2, 3]              # components of 3, 4, 5 voxels stay (12 rows) with the 5 rows outside
    assert kept_sizes('sizes_voxels4') == [5 + 4 + 5, 1 + 2 + 3, 3, 2]
    assert kept_sizes('sizes_points9') == kept_sizes('sizes_voxels3') and kept_sizes('sizes_points10') == kept_sizes('sizes_voxels4')
    assert kept_sizes('sizes_both') == [5 + 4 + 5, 6, 3, 2]                          # 12 points = 4 voxels
    assert kept_sizes('sizes_everything') == [5, 15, 5, 0] and kept_sizes('sizes_nothing') == [20, 0, 0, 5]
    assert kept_sizes('sizes_dry_run') == kept_sizes('sizes_voxels4') and _restate('sizes_dry_run')['keys'].shape[0] == 20
    gone = _restate('sizes_everything')
    assert gone['acc'][0].tolist() == [1] * 5 and gone['pierced'].tolist() == [51, 52, 53, 54, 55]    # the rows outside the filter, records and rays intact
    masked = _restate('sizes_mask')                                               # the mask cuts 5 -> 4 and 4 -> 1 + 2: only the 4 of the former 5 is left
    assert masked['voxels'] == [1, 2, 3, 1, 2, 4] and masked['remove_counters'] == [5 + 2 + 4, 9, 5, 1]
    assert {rref.coord_of(int(k)) for k in masked['keys']} >= {(50, 0, 0), (40, 1, 0)}


def test_floating_blobs_survive_prune_and_leave_with_their_component():
    """The gap this row closes, on the restatement alone: every blob voxel has enough neighbours for prune(min_neighbors=4), and
    remove_components(min_voxels=100) removes exactly the blob voxels."""
    _, blobs = _blob_scene()
    r, _ = tp._copy(*_scene('blobs'))
    before = set(rref.coord_of(k) for k in r.rec)
    assert len(blobs) == 135 and set(blobs) <= before
    why, k = rref.reasons(r, None, min_neighbors=4, radius=1)
    assert all(why[c] == rref.KEPT and k[c] >= 8 for c in blobs)                  # prune keeps every blob voxel
    res = cref.components(r, radius=1)
    assert sorted(res['voxels'])[:5] == [27] * 5 and res['counters'][4] >= 6
    assert cref.remove_components(r, None, min_voxels=100, radius=1)[1] == 135
    assert before - set(rref.coord_of(k) for k in r.rec) == set(blobs)            # the blobs and no sheet voxel


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_components_workspace_bytes', 'pcacc_accum_components', 'pcacc_accum_remove_components'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C11. ' in header and len(native._PROTOTYPES['pcacc_accum_components']) == 26 and len(native._PROTOTYPES['pcacc_accum_remove_components']) == 26
    for word, value in (('COUNTERS', 7), ('ROWS', 0), ('PARTICIPATING', 1), ('OUTSIDE', 2), ('MASKED', 3), ('K', 4), ('LARGEST', 5), ('STATUS', 6), ('OK', 0),
                        ('BAD_MASK', 1), ('GAVE_UP', 2), ('REMOVE_COUNTERS', 4), ('REMOVE_KEPT', 0), ('REMOVE_SMALL', 1), ('REMOVED', 2), ('SURVIVED', 3)):
        assert ('#define PCACC_COMPONENTS_%s %d\n' % (word, value)) in header and getattr(native, 'COMPONENTS_' + word) == value, word
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = open(os.path.join(csrc, 'accum_components.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_prune.h"', '#include "union_find.h"']
    assert all(w in text for w in ('accn_column(', 'accn_index(', 'accum_field(', 'accn_centroid(', 'accum_unkey('))
    kernels = open(os.path.join(csrc, 'accum_components.hip')).read()
    assert all(w in kernels for w in ('accr_move_row(', 'accum_merge_dst(', 'accn_rows_launch(', 'uf_union_bounded('))
    assert '#include "union_find.h"' in open(os.path.join(csrc, 'cluster.hip')).read()          # one copy of the union-find
    assert open(os.path.join(csrc, 'union_find.h')).read().count('int uf_find(') == 1 and 'int uf_find(' not in open(os.path.join(csrc, 'cluster.hip')).read()
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    for call in (cpu.components, lambda **kw: cpu.remove_components(min_voxels=2, **kw)):
        with pytest.raises(native.NativeError):
            call()
        with pytest.raises(native.NativeError):
            call(mask=torch.ones(3, dtype=torch.bool))                           # a CPU tensor
        for bad in (dict(radius=0), dict(radius=4), dict(mask=torch.ones(3, 1, dtype=torch.bool)), dict(mask=torch.ones(3)), dict(mask=[1, 0, 1]),
                    dict(mask=np.ones(3, bool)), dict(max_moving_fraction=float('nan'))):
            with pytest.raises(ValueError):                                      # before any call: the device is never asked
                call(**bad)
    for bad in (dict(), dict(min_voxels=-1), dict(min_points=-2), dict(min_voxels=1, min_points=-1)):
        with pytest.raises(ValueError):
            cpu.remove_components(**bad)
    cpu_tables = (torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(native.NativeError):
        native.accum_components(cpu_tables, 0, 1, None, None, 1)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
POISON = 77


def _native_components(m, mask, radius, min_count=1, max_moving_fraction=None):
    """pcacc_accum_components into poisoned tables of num_voxels rows -> host arrays sliced to kept and K, and the rows behind them."""
    from pcaccumulation_amd import native
    n = m.num_voxels
    out = {name: torch.full((n,) + shape, POISON, dtype=dtype, device=DEV) for name, dtype, shape in native.COMPONENTS_FIELDS}
    counters = torch.full((7,), POISON, dtype=torch.int64, device=DEV)
    res = native.accum_components(m._cur, n, min_count, max_moving_fraction, None if mask is None else torch.from_numpy(mask).to(DEV), radius, out=out,
                                  counters=counters)
    c = res['counters'].tolist()
    kept, k = c[0] - c[2], c[4]
    got = {name: res[name][:(kept if name == 'label' else k)].cpu().numpy() for name, _, _ in native.COMPONENTS_FIELDS}
    behind = all(bool((res[name][(kept if name == 'label' else k):] == POISON).all()) for name, _, _ in native.COMPONENTS_FIELDS)
    return dict(got, counters=c), behind, res


def _device_case(host_exe, tmp_path, name, scene, args):
    from pcaccumulation_amd import native
    host = _host(host_exe, tmp_path, name)
    m = tp._device_cloud(*_scene(scene))
    before, state = ah.snapshot(m), m._state.tolist()
    mask = _mask(scene, args)
    got, behind, raw = _native_components(m, mask, args['radius'], **_filter(args))
    _assert_components_equal(got, host, name)
    assert behind and got['counters'][6] != cref.GAVE_UP, name                    # rows behind kept / K are not written
    ah.assert_unchanged(m, before, name)                                         # components() leaves keys, records, stamps, sidecar, state, num_voxels
    again, _, _ = _native_components(m, mask, args['radius'], **_filter(args))
    assert all(np.array_equal(again[f].view(np.uint8) if f != 'counters' else again[f], got[f].view(np.uint8) if f != 'counters' else got[f]) for f in got), name
    call = dict(min_voxels=args.get('min_voxels') or None, min_points=args.get('min_points') or None, radius=args['radius'],
                mask=None if mask is None else torch.from_numpy(mask).to(DEV), **_filter(args))
    if call['min_voxels'] is None and call['min_points'] is None:
        call['min_voxels'] = 0
    if host['counters'][6] == cref.BAD_MASK:
        for dry in (True, False):
            with pytest.raises(ValueError):
                m.remove_components(dry_run=dry, **call)
            ah.assert_unchanged(m, before, name)
        with pytest.raises(ValueError):
            m.components(radius=args['radius'], mask=call['mask'], **_filter(args))
        return
    res = m.components(radius=args['radius'], mask=call['mask'], **_filter(args))
    assert all(torch.equal(res[f], raw[f][:res[f].shape[0]]) for f in res) and res['label'].shape[0] == len(host['label']), name
    dry = m.remove_components(dry_run=True, **call)
    want = dict(zip(cref.REMOVE_COUNTERS + cref.COUNTERS[:6], host['remove_counters'] + host['counters'][:6]))
    assert dry == want and all(type(v) is int for v in dry.values()), name
    ah.assert_unchanged(m, before, name)                                         # dry_run: records, sidecar, num_voxels and the state words stay
    if args.get('dry_run'):
        return
    assert m.remove_components(**call) == want, name
    n = want['kept']
    keys, acc, stamps = m._cur
    t = lambda a: torch.from_numpy(a).to(DEV)
    assert m.num_voxels == n and torch.equal(keys[:n], t(host['keys'])) and torch.equal(acc[:, :n], t(host['acc'])), name
    assert torch.equal(stamps[:, :n], t(host['stamps'])) and (m._pierced is None) == (host['pierced'] is None), name
    if host['pierced'] is not None:
        assert m._pierced.shape[0] == m.capacity and torch.equal(m._pierced[:n], t(host['pierced'])), name
    state[native.ACCUM_NUM_VOXELS] = n
    assert m._state.tolist() == state, name                                       # the state word is set on the device, the others are left alone


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    _device_case(host_exe, tmp_path, name, *CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(BIG))
def test_kernel_on_76981_voxels_gpu(host_exe, tmp_path, name):
    _device_case(host_exe, tmp_path, name, 'wavy_blobs', BIG[name])
    host = _host(host_exe, tmp_path, name)
    assert host['counters'][5] > 50000 and host['remove_counters'][2] >= 1       # the sheet (70 % of it under the mask) is one component; blobs leave


@pytest.mark.gpu
def test_identities_gpu():
    r, pierced = _scene('rows257')
    m = tp._device_cloud(r, pierced)
    cloud = m.extract(**FILTER)
    mask = torch.from_numpy(_mask('rows257', dict(mask=('random', 4), **FILTER))).to(DEV)
    one = m.components(radius=1, mask=mask, **FILTER)
    c = one['counters'].tolist()
    part = one['label'] >= 0
    assert int(one['voxels'].sum()) == c[1] == int(part.sum()) and torch.equal(part, mask != 0)
    assert int(one['points'].sum()) == int(cloud['count'][part].sum()) and int(one['moving'].sum()) == int(cloud['moving'][part].sum())
    rows = one['first_row'].long()
    assert torch.equal(one['label'][rows].long(), torch.arange(c[4], device=DEV)) and bool((rows[1:] > rows[:-1]).all())
    lab, coords = one['label'][part].long(), cloud['coords'][part]
    assert bool((coords >= one['lo'][lab]).all()) and bool((coords <= one['hi'][lab]).all())
    for k in range(c[4]):                                                         # each face of the box is attained
        mine = coords[lab == k]
        assert torch.equal(mine.min(0).values, one['lo'][k]) and torch.equal(mine.max(0).values, one['hi'][k]), k
        assert int(cloud['t_first'][part][lab == k].min()) == int(one['t_first'][k]) and int(cloud['t_last'][part][lab == k].max()) == int(one['t_last'][k])
    ones, none = m.components(radius=2, mask=torch.ones_like(mask), **FILTER), m.components(radius=2, **FILTER)
    assert all(torch.equal(ones[f], none[f]) for f in none)
    fine, coarse = m.components(radius=1), m.components(radius=2)                 # every r = 1 component maps into exactly one r = 2 component
    pairs = torch.unique(torch.stack([fine['label'], coarse['label']], 1), dim=0)
    assert pairs.shape[0] == fine['voxels'].shape[0] and coarse['voxels'].shape[0] <= fine['voxels'].shape[0]
    snap = ah.snapshot(m)
    res = m.remove_components(min_voxels=1)
    assert res['small'] == 0 and res['kept'] == 257
    ah.assert_unchanged(m, snap, 'min_voxels = 1')                               # a bit-identical map
    m, k = tp._device_cloud(*_scene('sizes')), 4                                  # components of 2 .. 6 voxels: no filter, no mask
    before = m.components(radius=1)
    stay = before['voxels'] >= k
    assert 0 < int(stay.sum()) < stay.shape[0]
    res = m.remove_components(min_voxels=k)
    after = m.components(radius=1)
    assert res['components_kept'] == int(stay.sum()) and res['small'] == int(before['voxels'][~stay].sum())
    for f in ('voxels', 'points', 'moving', 'sum_q', 'centroid', 'lo', 'hi', 't_first', 't_last'):
        assert torch.equal(after[f], before[f][stay]), f                          # the earlier list restricted to voxels >= k, in order


@pytest.mark.gpu
def test_floating_blobs_leave_the_map_gpu():
    sheet, blobs = _blob_scene()
    r, _ = tp._copy(*_scene('blobs'))
    m = tp._device_cloud(r, None)
    res = m.prune(min_neighbors=4, radius=1)
    assert [res[f] for f in rref.NAMES] == rref.prune(r, None, min_neighbors=4, radius=1)
    left = {tuple(c) for c in m.extract()['coords'].cpu().tolist()}
    assert set(blobs) <= left                                                     # the real prune keeps every blob voxel
    res = m.remove_components(min_voxels=100)
    assert [res[f] for f in cref.REMOVE_COUNTERS] == cref.remove_components(r, None, min_voxels=100, radius=1) and res['small'] == 135
    tp._assert_equals_restatement(m, r, None, 'blobs removed')
    cloud, nrm = m.extract(), m.normals(radius=1, min_neighbors=5)
    coords = {tuple(c) for c in cloud['coords'].cpu().tolist()}
    assert left - coords == set(blobs) and nrm['normals'].shape[0] == len(coords) == m.num_voxels


@pytest.mark.gpu
def test_objects_on_the_ground_gpu():
    ground = {(x, y, 0): (2, 0, 0, 0) for x in range(-10, 30) for y in range(-8, 8)}
    boxes = [((-6, -5, 1), (-3, -2, 6)), ((4, 0, 1), (9, 3, 3)), ((20, -6, 1), (22, 5, 9))]
    rows = dict(ground)
    for lo, hi in boxes:
        rows.update({(x, y, z): (3, 1, 1, 2) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)})
    r = ah.records(0.1, rows)
    m = tp._device_cloud(r, None)
    whole = m.components()
    assert whole['voxels'].tolist() == [len(rows)] and whole['counters'].tolist()[4:] == [1, len(rows), 0]
    cloud = m.extract()
    mask = cloud['points'][:, 2] > 0.1                                            # cut the ground away by height
    res = m.components(mask=mask)
    want = cref.components(r, radius=1, mask=(cloud['points'][:, 2] > 0.1).cpu().tolist())
    assert res['counters'].tolist() == want['counters'] and want['counters'][4] == 3 and want['counters'][3] == len(ground)
    assert res['lo'].tolist() == [list(b[0]) for b in boxes] == want['lo'] and res['hi'].tolist() == [list(b[1]) for b in boxes] == want['hi']
    assert res['voxels'].tolist() == want['voxels'] and res['label'].cpu().tolist() == want['label']
    centroid = res['centroid'].double()
    assert bool((centroid >= res['lo'].double() * 0.1).all()) and bool((centroid <= (res['hi'].double() + 1) * 0.1).all())


@pytest.mark.gpu
def test_life_cycle_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m, r, pierced = AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1), {}

    def check(what, **args):
        res, want = m.components(**args), cref.components(r, **args)
        got = {f: res[f].cpu().numpy() for f in res if f != 'counters'}
        _assert_components_equal(dict(got, counters=res['counters'].tolist()), want, what)

    slab = [(x, y, z) for x in (5, 6, 7) for y in range(-2, 3) for z in (-1, 0, 1)]
    pair = [(6, 8, 0), (6, 9, 0)]
    tp._both_add(m, r, slab + pair + [(-9, 0, 0)], 0)
    check('first add', radius=1)
    tp._both_see(m, r, pierced, [(20, y, 0) for y in (-2, 0, 3)] + [(20, 27, 0)], 1)   # rays through the slab and through the pair
    assert pierced.get((6, 8, 0), 0) >= 1
    res = m.remove_components(min_voxels=3)
    assert [res[f] for f in cref.REMOVE_COUNTERS] == cref.remove_components(r, pierced, min_voxels=3, radius=1) and res['small'] == 3
    tp._assert_equals_restatement(m, r, pierced, 'first removal')
    assert m.capacity == 64 and m.dropped == 0
    tp._both_add(m, r, [(6, 8, 0), (6, 8, 0), (30, 1, 1)], 2)                      # a removed voxel is seen again
    tp._assert_equals_restatement(m, r, pierced, 'add after removal')
    back = r.rec[rref.key_of((6, 8, 0))]
    assert back[0] == 2 and back[5:] == [2, 2] and pierced.get((6, 8, 0), 0) == 0  # the new points only, fresh stamps, no rays
    row = int(np.searchsorted(m.records()[0], rref.key_of((6, 8, 0))))
    assert m.records()[1][0, row] == 2 and m.records()[2][:, row].tolist() == [2, 2] and int(m._pierced[row]) == 0
    big = [(x, y, z) for x in range(-8, 8) for y in range(-8, 8) for z in range(40, 56)]        # 4096 new voxels: the tables grow
    tp._both_add(m, r, big, 3)
    assert m.capacity >= 4096
    check('after growth', radius=2, min_count=1)
    path = os.path.join(str(tmp_path), 'components.npz')
    m.save(path)
    loaded = AccumulatedCloud.load(path, DEV)
    a, b = m.components(radius=1), loaded.components(radius=1)
    assert all(torch.equal(a[f], b[f]) for f in a)
    res = loaded.remove_components(min_points=3, radius=1)
    assert [res[f] for f in cref.REMOVE_COUNTERS] == cref.remove_components(r, pierced, min_points=3, radius=1) and res['small'] >= 2
    tp._assert_equals_restatement(loaded, r, pierced, 'after load')


@pytest.mark.gpu
def test_components_on_the_model_forward_gpu(golden, host_exe, tmp_path):
    """components() after add_results on the model_tiny_test forward: the counters are consistent and the labels equal the g++ build on the map's
    records().  Nothing more is claimed."""
    from helpers import make_batch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    from pcaccumulation_amd.config import default_config
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
    res = m.components(radius=1)
    c = res['counters'].tolist()
    assert c[0] == m.num_voxels == c[1] and c[2] == c[3] == 0 and c[6] == 0 and int(res['voxels'].sum()) == c[1] and int(res['voxels'].max()) == c[5]
    host = _run_host(host_exe, tmp_path, 'forward', m.records(), None, None, radius=1)
    assert np.array_equal(res['label'].cpu().numpy(), host['label']) and c == host['counters']


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_gpu():
    from pcaccumulation_amd import native
    r, pierced = _scene('rows65')
    m = tp._device_cloud(r, pierced)
    snap = ah.snapshot(m)
    out = {name: torch.full((65,) + shape, POISON, dtype=dtype, device=DEV) for name, dtype, shape in native.COMPONENTS_FIELDS}
    counters = torch.full((7,), POISON, dtype=torch.int64, device=DEV)
    good = dict(tables=m._cur, m=65, min_count=1, max_moving_fraction=None, mask=None, radius=1, out=out, counters=counters)
    for bad in (dict(m=m.capacity + 1, out={k: torch.full((m.capacity + 1,) + tuple(v.shape[1:]), POISON, dtype=v.dtype, device=DEV) for k, v in out.items()}),
                dict(radius=0), dict(radius=4)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_components(**dict(good, **bad))
    l = native.lib()
    keys, acc, stamps, cap = native._accum_tables(m._cur, 'test')
    ptrs = [native._dev(out[name]) for name, _, _ in native.COMPONENTS_FIELDS]
    ws = native._workspace(l.pcacc_accum_components_workspace_bytes, m._cur[0].device, 65)
    call = lambda m_=65, mask=None, mask_rows=0, radius=1, p=ptrs, k=keys, w=native._dev(ws), wb=ws.numel(): l.pcacc_accum_components(
        k, acc, stamps, cap, m_, 1, 0, 0.0, mask, mask_rows, radius, *p, native._dev(counters), w, wb, native._stream())
    assert call(m_=-1) == call(mask_rows=-1) == call(k=None) == call(p=[None] + ptrs[1:]) == call(p=ptrs[:-1] + [None]) == call(wb=64) == call(w=None) == -1
    assert call(mask=None, mask_rows=3) == -1
    size = native.ctypes.c_size_t(0)
    assert l.pcacc_accum_components_workspace_bytes(-1, native.ctypes.byref(size)) == -1 and l.pcacc_accum_components_workspace_bytes(65, None) == -1
    first = native.accum_components(m._cur, 65, 1, None, None, 1)
    tabs = tuple(torch.full_like(t, POISON) for t in m._cur)
    pout = torch.full_like(m._pierced, POISON)
    rcounters = torch.full((4,), POISON, dtype=torch.int64, device=DEV)
    good = dict(tables_in=m._cur, m=65, pierced_in=m._pierced, min_count=1, max_moving_fraction=None, first=first, min_voxels=2, min_points=0, dry_run=False,
                tables_out=tabs, pierced_out=pout, counters=rcounters, state=m._state)
    small = tuple(t[..., :64].contiguous() for t in tabs)
    for bad in (dict(min_voxels=-1), dict(min_points=-1), dict(tables_out=small, pierced_out=pout[:64].contiguous()), dict(tables_out=m._cur),
                dict(pierced_out=m._pierced), dict(tables_out=(tabs[0], m._cur[1], tabs[2])), dict(tables_out=None, pierced_out=None),
                dict(pierced_out=None), dict(state=None)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_remove_components(**dict(good, **bad))
    torch.cuda.synchronize()
    ah.assert_unchanged(m, snap, 'bad arguments')
    assert all(bool((t == POISON).all()) for t in tuple(out.values()) + tabs + (pout, counters, rcounters))
    empty = {name: torch.zeros((0,) + shape, dtype=dtype, device=DEV) for name, dtype, shape in native.COMPONENTS_FIELDS}
    zero = native.accum_components(m._cur, 0, 1, None, None, 1, out=empty, counters=counters)        # m = 0: the zero counters and nothing else
    native.accum_remove_components(**dict(good, m=0, first=zero))
    assert counters.tolist() == [0] * 7 and rcounters.tolist() == [0] * 4 and all(bool((t == POISON).all()) for t in tabs + (pout,))
    ah.assert_unchanged(m, snap, 'm = 0')
    for bad in (dict(radius=4), dict(mask=torch.ones(65, dtype=torch.float32, device=DEV)), dict(mask=torch.ones(65, 1, dtype=torch.bool, device=DEV))):
        with pytest.raises(ValueError):
            m.components(**bad)
        with pytest.raises(ValueError):
            m.remove_components(min_voxels=2, **bad)
    for bad in (dict(), dict(min_voxels=-1), dict(min_points=-1)):
        with pytest.raises(ValueError):
            m.remove_components(**bad)
    with pytest.raises(native.NativeError):
        m.components(mask=torch.ones(65, dtype=torch.bool))
    with pytest.raises(ValueError):
        m.components(mask=torch.ones(64, dtype=torch.bool, device=DEV))           # BAD_MASK, found on the device
    ah.assert_unchanged(m, snap, 'ValueError')
