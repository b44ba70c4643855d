"""Scan-to-map registration of the accumulated scene cloud (include/pcacc.h C6): AccumulatedCloud.register / register_results.

CPU leg: csrc/accum_register.h -- the code the kernels run -- built with g++ (-ffp-contract=off, every table index assert-checked, poison behind row m)
runs the whole iteration loop against the numpy restatement tests/accumulate_register_reference.py (a dict of coordinates, numpy's sums,
np.linalg.solve): correspondence rows, counts, status and iterations equal; pose, fitness and rmse inside PARITY_BOUND.
GPU leg: the kernels against the host build BIT FOR BIT at max_iter = 1 and at convergence on every scene of the CPU leg; reproducibility; the map
untouched; drifted windows registered before their add; argument errors; the model tie-in."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_reference as ref
import accumulate_register_reference as rref
from accumulate_helpers import DEV
from helpers import ROOT
from pcaccumulation_amd.config import default_config

MAX_ITER = 20
# Pose (largest entry of the 3 x 4 difference), fitness and rmse of the host build against the restatement: ten times the largest difference measured
# on the CPU over every scene below, floored at 1e-9.  Measured (profiles/accum_register_parity.txt): 4.9e-15 after one update, 3.1e-16 at convergence
# -- the floor decides.
PARITY_BOUND = 1e-9
SPHERE_CENTRE = np.array([0.3, -0.2, 0.1])


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
TRUE_POSE = ah.rot_xyz(np.deg2rad(0.6), np.deg2rad(-0.5), np.deg2rad(0.7), (0.02, -0.015, 0.017))      # about 1 degree and 0.3 voxel of 0.1


def _into_scan_frame(world, pose):
    """The scan whose points `pose` maps onto `world`."""
    inv = np.linalg.inv(pose)
    return (world @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


def _sphere(seed, n):
    rs = np.random.RandomState(seed)
    d = rs.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return SPHERE_CENTRE + d * (1.5 + rs.normal(0, 0.005, n))[:, None]


def _bound_voxels():
    """Section 9d's index-bound clusters and their decoys (accumulate_helpers.bound_voxels) as int64 arrays [N,3]."""
    return tuple(np.array(v, np.int64) for v in ah.bound_voxels())


def _tie_sheet():
    """Voxel size 2^-3: a 6 x 6 sheet of voxel centres, every number exact.  Interior voxels get the normal (0, 0, 1)."""
    return ah.centres([(x, y, 0) for x in range(6) for y in range(6)], 0.125)


_BAD_ROWS = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [32768.0, 0, 0], [0, -32768.0, 0]], np.float32)


def _map_adds(name):
    """-> (voxel_size, [(points, moving or None, stamp)]) of the map a case registers against."""
    if name == 'corner':
        return 0.1, [(ah.corner(11, 9000).astype(np.float32), None, 0)]
    if name == 'plane':                                                          # z is one float32 for every point: every valid normal is exactly (0, 0, 1)
        rs = np.random.RandomState(5)
        xy = rs.uniform(-1.0, 1.0, (6000, 2))
        return 0.1, [(np.concatenate([xy, np.full((6000, 1), 0.05)], 1).astype(np.float32), None, 0)]
    if name == 'sphere':
        return 0.1, [(_sphere(7, 40000).astype(np.float32), None, 0)]
    if name == 'bound':
        cluster, decoys = _bound_voxels()
        return 0.01, [(ah.centres(np.concatenate([cluster, decoys]), 0.01), None, 0)]
    if name == 'tie':
        return 0.125, [(_tie_sheet(), None, 0)]
    if name == 'flagged':                                                        # the corner with points predicted moving, two stamps
        pts = ah.corner(11, 9000).astype(np.float32)
        mv = np.random.RandomState(8).uniform(0, 1, pts.shape[0]) < 0.01
        perm = np.random.RandomState(9).permutation(pts.shape[0])
        a, b = perm[:14000], perm[14000:]
        return 0.1, [(pts[a], mv[a], 3), (pts[b], mv[b], 1)]
    assert name == 'empty'
    return 0.1, []


def _corner_scan(n_per_sheet=1300, seed=12):
    return _into_scan_frame(ah.corner(seed, n_per_sheet), TRUE_POSE)


def _case(name):
    """-> dict: map (a _map_adds name), points [n,3] f32, and the arguments of register that differ from the defaults."""
    scan = _corner_scan()
    if name == 'corner':
        return dict(map='corner', points=scan)
    if name == 'corner_init':                                                    # a start that is not the identity, and a tighter gate
        init = ah.rot_xyz(0, 0, np.deg2rad(0.3), (0.01, 0.0, 0.0))
        return dict(map='corner', points=scan, init_pose=init, max_distance=0.08)
    if name == 'plane':
        rs = np.random.RandomState(6)
        pts = np.concatenate([rs.uniform(-0.8, 0.8, (2000, 2)), 0.05 + rs.normal(0, 0.01, (2000, 1))], 1)
        return dict(map='plane', points=_into_scan_frame(pts, ah.rot_xyz(0.004, -0.003, 0, (0, 0, 0.01))), init_pose=ah.rot_xyz(0, 0, 0.002, (0.001, 0.002, 0)))
    if name == 'sphere':
        vp = SPHERE_CENTRE[None]
        return dict(map='sphere', points=_into_scan_frame(_sphere(17, 4000), TRUE_POSE), viewpoints=vp)
    if name == 'bound':                                                          # the scan sits in the boundary voxels themselves
        cluster, _ = _bound_voxels()
        rs = np.random.RandomState(3)
        pts = (cluster + 0.5 + rs.uniform(-0.45, 0.45, cluster.shape)) * 0.01
        return dict(map='bound', points=pts.astype(np.float32), max_iter=1)
    if name == 'tie':                                                            # midway between voxels x = 2 | 3, and between y = 2 | 3 as well: four equal d2
        pts = np.array([[0.375, 0.3125, 0.09], [0.375, 0.375, 0.08], [0.3125, 0.3125, 0.0625], [0.5, 0.375, 0.05]], np.float32)
        return dict(map='tie', points=pts, max_iter=1)
    if name.startswith('n'):                                                     # scan sizes around the group of 64 and the slot of 256
        n = int(name[1:])
        return dict(map='corner', points=scan[np.random.RandomState(n).permutation(scan.shape[0])[:n]])
    if name == 'bad_first':
        return dict(map='corner', points=np.concatenate([_BAD_ROWS, scan[:300]]))
    if name == 'bad_last':
        return dict(map='corner', points=np.concatenate([scan[:300], _BAD_ROWS]))
    if name == 'bad_alone':
        return dict(map='corner', points=_BAD_ROWS[:1])
    if name == 'some_moving':
        return dict(map='corner', points=scan, moving=np.random.RandomState(4).uniform(0, 1, scan.shape[0]) < 0.3)
    if name == 'all_moving':
        return dict(map='corner', points=scan[:500], moving=np.ones(500, bool))
    if name == 'empty_map':
        return dict(map='empty', points=scan[:200])
    if name == 'empty_scan':
        return dict(map='corner', points=np.zeros((0, 3), np.float32))
    if name == 'keeps_nothing':
        return dict(map='corner', points=scan[:200], min_count=10 ** 6)
    assert name == 'flagged'
    return dict(map='flagged', points=scan, min_count=2, max_moving_fraction=0.0)


RAGGED = 256 * 3 + 37
SIZES = ('n1', 'n63', 'n64', 'n65', 'n257', 'n%d' % RAGGED)
SCENES = ('corner', 'corner_init', 'plane', 'sphere', 'bound', 'tie', 'flagged', 'some_moving')
EDGES = ('bad_first', 'bad_last', 'bad_alone', 'all_moving', 'empty_map', 'empty_scan', 'keeps_nothing')
ALL_CASES = SCENES + SIZES + EDGES
_maps, _host_cache, _want_cache = {}, {}, {}


def _ref_map(name):
    """The restatement's map, built once and shared (never modified)."""
    if name not in _maps:
        vs, adds = _map_adds(name)
        r = ref.ReferenceMap(vs)
        for pts, mv, stamp in adds:
            r.add(pts, None, mv, stamp)
        _maps[name] = r
    return _maps[name]


def _args(case, max_iter):
    a = dict(init_pose=None, moving=None, max_distance=None, max_iter=max_iter, min_count=1, max_moving_fraction=None, radius=1, min_neighbors=5,
             viewpoints=None, stamp_base=0)
    a.update({k: v for k, v in case.items() if k not in ('map', 'points')})
    a['max_iter'] = min(a['max_iter'], max_iter)
    return a


# ---- the host build ----------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_register_host_driver', 'accr')


def _run_host(exe, tmp_path, records, voxel_size, points, a, spare=3):
    """The g++ build of accum_register.h on integer records (every assert of the driver aborts it)."""
    keys, acc, stamps = records
    m, n = keys.shape[0], points.shape[0]
    vp = np.zeros((0, 3)) if a['viewpoints'] is None else np.ascontiguousarray(a['viewpoints'], np.float64).reshape(-1, 3)
    frac = a['max_moving_fraction']
    head = [m, max(m + spare, 1), a['min_count'], 0 if frac is None else 1, a['radius'], a['min_neighbors'], vp.shape[0], a['stamp_base'], n,
            0 if a['moving'] is None else 1, a['max_iter'], 0 if a['init_pose'] is None else 1]
    raw = ah.run_driver(exe, tmp_path, 'r%d' % len(os.listdir(str(tmp_path))), np.array(head, np.int64),
                        np.array([0.0 if frac is None else frac, voxel_size, voxel_size if a['max_distance'] is None else a['max_distance']], np.float64),
                        ah.map_bytes(keys, acc, stamps), vp, np.ascontiguousarray(points, np.float32),
                        b'' if a['moving'] is None else (np.asarray(a['moving']) != 0).astype(np.uint8),
                        b'' if a['init_pose'] is None else np.ascontiguousarray(a['init_pose'], np.float64), suffix='.bin')
    res = {'pose': np.frombuffer(raw, np.float64, 16).reshape(4, 4), 'fitness': np.frombuffer(raw, np.float64, 1, 128)[0],
           'rmse': np.frombuffer(raw, np.float64, 1, 136)[0]}
    res['iterations'], res['status'], res['correspondences'] = (int(x) for x in np.frombuffer(raw, np.int32, 3, 144))
    v = int(np.frombuffer(raw, np.int64, 1, 156)[0])
    tables, off = ah.unpack(raw, 164, [('normals32', np.float32, (v, 3)), ('flags', np.uint8, (v,)), ('first', np.int64, (n,)), ('last', np.int64, (n,)),
                                       ('evaluations', np.int64, ())])
    assert off == len(raw)
    return dict(res, **tables)


def _host(exe, tmp_path, name, max_iter):
    if (name, max_iter) not in _host_cache:
        case = _case(name)
        r = _ref_map(case['map'])
        _host_cache[(name, max_iter)] = _run_host(exe, tmp_path, r.records(), r.voxel_size, case['points'], _args(case, max_iter))
    return _host_cache[(name, max_iter)]


def _want(exe, tmp_path, name, max_iter):
    """The restatement on the same inputs, with the host build's float32 normals (C5's own tests cover those)."""
    if (name, max_iter) not in _want_cache:
        case = _case(name)
        a = _args(case, max_iter)
        host = _host(exe, tmp_path, name, max_iter)
        _want_cache[(name, max_iter)] = rref.register(_ref_map(case['map']), host['normals32'], host['flags'], case['points'], a['init_pose'], a['moving'],
                                                      a['max_distance'], a['max_iter'], a['min_count'], a['max_moving_fraction'])
    return _want_cache[(name, max_iter)]


def _pose_err(a, b):
    return float(np.abs(np.asarray(a)[:3] - np.asarray(b)[:3]).max())


def _compare(got, want, what):
    """Integers equal, floats inside PARITY_BOUND.  -> the three differences."""
    for k in ('iterations', 'status', 'correspondences'):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got['last'], want['last']), (what, np.flatnonzero(got['last'] != want['last'])[:8])
    assert np.array_equal(got['pose'][3], [0, 0, 0, 1])
    diffs = (_pose_err(got['pose'], want['pose']), abs(got['fitness'] - want['fitness']), abs(got['rmse'] - want['rmse']))
    print('parity %-14s pose %.3e fitness %.3e rmse %.3e (status %d, %d updates, %d correspondences)'
          % ((what,) + diffs + (got['status'], got['iterations'], got['correspondences'])))
    assert max(diffs) <= PARITY_BOUND, (what, diffs)
    return diffs


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SCENES + SIZES)
def test_host_build_against_the_restatement(host_exe, tmp_path, name):
    """One update, then convergence: the same rows and counts, pose / fitness / rmse inside the bound."""
    for max_iter in (1, MAX_ITER):
        got, want = _host(host_exe, tmp_path, name, max_iter), _want(host_exe, tmp_path, name, max_iter)
        assert np.array_equal(got['first'], want['first']), (name, np.flatnonzero(got['first'] != want['first'])[:8])
        assert int((got['first'] >= 0).sum()) == int((want['first'] >= 0).sum())
        _compare(got, want, '%s/%d' % (name, max_iter))
        assert got['evaluations'] == got['iterations'] + 1 or got['status'] & ~rref.MAX_ITER
    n = _case(name)['points'].shape[0]
    if name in ('corner', 'sphere', 'flagged', 'some_moving', 'n%d' % RAGGED):
        assert got['status'] == 0 and 2 <= got['iterations'] < MAX_ITER and got['fitness'] > 0.5, (got['status'], got['iterations'], got['fitness'])
    if name == 'n1':
        assert got['status'] == rref.DEGENERATE and n == 1


def test_corner_pose_is_recovered(host_exe, tmp_path):
    """The recovered pose lies closer to the truth than init_pose does; how close is the restatement's own result, with the margin of the parity bound."""
    for name in ('corner', 'corner_init', 'flagged'):
        case = _case(name)
        init = np.eye(4) if case.get('init_pose') is None else case['init_pose']
        got, want = _host(host_exe, tmp_path, name, MAX_ITER), _want(host_exe, tmp_path, name, MAX_ITER)
        e_got, e_want, e_init = _pose_err(got['pose'], TRUE_POSE), _pose_err(want['pose'], TRUE_POSE), _pose_err(init, TRUE_POSE)
        print('%s: |pose - truth| %.3e (restatement %.3e), init %.3e' % (name, e_got, e_want, e_init))
        assert e_init > 0.01
        assert e_got < e_init and e_want < e_init
        assert e_got <= max(10 * e_want, 1e-9)
        assert e_want < 0.005                                                    # and the scene does pin the pose: inside half the sheets' noise (sigma 0.01)
        R = got['pose'][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0


def test_one_plane_alone_is_degenerate(host_exe, tmp_path):
    """Nothing constrains the translation inside the plane or the rotation about its normal: DEGENERATE, the pose is init_pose bit for bit."""
    case = _case('plane')
    for max_iter in (1, MAX_ITER):
        got = _host(host_exe, tmp_path, 'plane', max_iter)
        assert got['status'] == rref.DEGENERATE and got['iterations'] == 0
        assert got['pose'][:3].tobytes() == np.ascontiguousarray(case['init_pose'][:3]).tobytes()
        assert got['fitness'] == 0.0 and got['rmse'] == 0.0 and got['correspondences'] > 1000
    valid = (got['flags'] & 3) == 0
    assert valid.sum() > 300 and np.all(got['normals32'][valid] == np.array([0, 0, 1], np.float32))


def test_index_bound_ignores_decoys(host_exe, tmp_path):
    """Scan points in voxels that touch +-2^20: offsets that leave the grid are skipped before a key is formed (the driver's asserts stay silent), and
    a decoy sitting where the overflowed key would land is never a candidate: rows and counts equal the dict restatement's."""
    got, want = _host(host_exe, tmp_path, 'bound', 1), _want(host_exe, tmp_path, 'bound', 1)
    cluster, decoys = _bound_voxels()
    keys = _ref_map('bound').records()[0]
    coords = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - ref.BIAS
    assert set(map(tuple, coords.tolist())) == set(map(tuple, cluster.tolist())) | set(map(tuple, decoys.tolist())) and len(decoys) >= 36
    assert np.array_equal(got['first'], want['first']) and got['correspondences'] == want['correspondences']
    matched = got['first'] >= 0
    assert matched.sum() >= 50                                                   # the clusters do have valid normals to match
    decoy_rows = {j for j, c in enumerate(coords.tolist()) if tuple(c) in set(map(tuple, decoys.tolist())) - set(map(tuple, cluster.tolist()))}
    assert decoy_rows and not (set(got['first'][matched].tolist()) & decoy_rows)


def test_ties_go_to_the_lowest_key(host_exe, tmp_path):
    got, want = _host(host_exe, tmp_path, 'tie', 1), _want(host_exe, tmp_path, 'tie', 1)
    keys = _ref_map('tie').records()[0]
    coords = (np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - ref.BIAS).tolist()
    # point 0: x midway between voxels 2 | 3; point 1: x and y midway (four equal distances); point 2: the same, in the plane; point 3: x between 3 | 4
    assert [coords[r] for r in got['first']] == [[2, 2, 0], [2, 2, 0], [2, 2, 0], [3, 2, 0]]
    assert np.array_equal(got['first'], want['first'])


@pytest.mark.parametrize('name', EDGES)
def test_edges_on_the_host_build(host_exe, tmp_path, name):
    """Invalid rows first, last and alone; all points moving; an empty map, an empty scan, a filter that keeps nothing."""
    case = _case(name)
    for max_iter in (1, MAX_ITER):
        got, want = _host(host_exe, tmp_path, name, max_iter), _want(host_exe, tmp_path, name, max_iter)
        assert np.array_equal(got['first'], want['first'])
        _compare(got, want, '%s/%d' % (name, max_iter))
    n = case['points'].shape[0]
    if name in ('bad_first', 'bad_last'):
        bad = slice(0, 5) if name == 'bad_first' else slice(n - 5, n)
        assert np.all(got['first'][bad] == -1) and np.all(got['last'][bad] == -1)
        assert got['status'] == 0 and got['correspondences'] > 250
        assert abs(got['fitness'] - got['correspondences'] / n) < 1e-15           # the invalid rows count in the denominator
        if name == 'bad_last':                                                   # rows behind the scan move no term to another position: the same bits
            plain = _run_host(host_exe, tmp_path, _ref_map('corner').records(), 0.1, _corner_scan()[:300], _args(dict(), MAX_ITER))
            assert plain['pose'].tobytes() == got['pose'].tobytes() and plain['correspondences'] == got['correspondences']
            assert plain['rmse'] == got['rmse'] and plain['fitness'] > got['fitness']
    else:
        bit = {'bad_alone': rref.NO_CORRESPONDENCE, 'all_moving': rref.NO_ELIGIBLE, 'empty_map': rref.NO_CANDIDATE,
               'empty_scan': rref.NO_ELIGIBLE, 'keeps_nothing': rref.NO_CANDIDATE}[name]
        assert got['status'] == bit and got['iterations'] == 0 and got['correspondences'] == 0
        assert got['fitness'] == 0.0 and got['rmse'] == 0.0 and got['pose'].tobytes() == np.eye(4).tobytes()
        assert np.all(got['first'] == -1)


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_register_workspace_bytes', 'pcacc_accum_register'):
        assert ('int %s(' % name) in header
        assert name in native.EXPORTS
    assert ' C6. ' in header
    for word, bit in (('NO_ELIGIBLE', 1), ('NO_CANDIDATE', 2), ('NO_CORRESPONDENCE', 4), ('DEGENERATE', 8), ('MAX_ITER', 16), ('BAD_TABLE', 32)):
        assert ('PCACC_REGISTER_%s %d' % (word, bit)) in header and getattr(native, 'REGISTER_' + word) == bit == getattr(rref, word)
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_register.h')).read()
    assert '#include <hip' not in text and 'PCACC_NO_CONTRACT' in text and 'PCACC_HD' in text
    assert callable(native.accum_register)
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).register(torch.zeros(4, 3))
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).register(np.zeros((4, 3), np.float32))
    cpu_tables = (torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(native.NativeError):
        native.accum_register(torch.zeros(4, 3), None, None, 0.1, 0.1, 5, cpu_tables, 0, 1, None, torch.zeros(0, 3), torch.zeros(0, dtype=torch.uint8))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
_device_maps = {}


def _device_map(name):
    """A device map per scene, shared: register does not modify it (a test below says so)."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    if name not in _device_maps:
        vs, adds = _map_adds(name)
        m = AccumulatedCloud(vs, DEV, 64)
        for pts, mv, stamp in adds:
            m.add(torch.from_numpy(pts).to(DEV), None, None if mv is None else torch.from_numpy(mv).to(DEV), stamp)
        _device_maps[name] = m
    return _device_maps[name]


def _register(m, case, max_iter):
    a = _args(case, max_iter)
    mv = None if a['moving'] is None else torch.from_numpy(np.asarray(a['moving'])).to(DEV)
    return m.register(torch.from_numpy(case['points']).to(DEV), a['init_pose'], mv, a['max_distance'], a['max_iter'], a['min_count'],
                      a['max_moving_fraction'], a['radius'], a['min_neighbors'], a['viewpoints'], a['stamp_base'])


def _assert_result_bits(res, host, what):
    assert sorted(res) == ['correspondences', 'fitness', 'iterations', 'pose', 'rmse', 'status']
    assert res['pose'].dtype == torch.float64 and tuple(res['pose'].shape) == (4, 4) and res['pose'].is_cuda
    assert res['fitness'].dtype == torch.float64 and res['rmse'].dtype == torch.float64 and res['fitness'].dim() == 0
    assert all(res[k].dtype == torch.int32 and res[k].dim() == 0 for k in ('iterations', 'status', 'correspondences'))
    got = {k: v.cpu().numpy() for k, v in res.items()}
    print('%s: status %d, %d updates, %d correspondences, fitness %.6f rmse %.6f' % (what, got['status'], got['iterations'], got['correspondences'],
                                                                                   got['fitness'], got['rmse']))
    for k in ('iterations', 'status', 'correspondences'):
        assert int(got[k]) == host[k], (what, k, int(got[k]), host[k])
    for k in ('pose', 'fitness', 'rmse'):
        assert got[k].tobytes() == np.asarray(host[k], np.float64).tobytes(), (what, k, got[k], host[k])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ALL_CASES)
def test_kernel_equals_the_host_build_bits_gpu(host_exe, tmp_path, name):
    """Same code, same float64 operations in the same order, no FMA contraction on either side: equal bytes, after one update and at convergence."""
    case = _case(name)
    m = _device_map(case['map'])
    for x, y in zip(m.records(), _ref_map(case['map']).records()):
        assert x.tobytes() == y.tobytes()
    for max_iter in (1, MAX_ITER):
        _assert_result_bits(_register(m, case, max_iter), _host(host_exe, tmp_path, name, max_iter), '%s/%d' % (name, max_iter))


@pytest.mark.gpu
def test_two_runs_are_equal_and_the_map_is_untouched_gpu():
    m = _device_map('corner')
    before = m.records()
    n_before, dropped = m.num_voxels, m.dropped
    case = _case('corner')
    a, b = _register(m, case, MAX_ITER), _register(m, case, MAX_ITER)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert int(a['status']) == 0 and int(a['iterations']) >= 2
    for x, y in zip(before, m.records()):
        assert x.tobytes() == y.tobytes()
    assert (m.num_voxels, m.dropped) == (n_before, dropped)


@pytest.mark.gpu
def test_registering_drifted_windows_before_their_add_gpu(host_exe, tmp_path):
    """Three windows of the corner; the poses that come with windows 1 and 2 have drifted (the true pose is TRUE_POSE-like, the given one is off by
    about a degree and a third of a voxel).  Adding with the drifted poses puts every wall into neighbouring voxels; registering each window against
    the map so far before its add gives strictly fewer voxels -- at most what the restatement, run the same way, gets."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    truth = [np.eye(4), TRUE_POSE, ah.rot_xyz(np.deg2rad(-0.7), np.deg2rad(0.4), np.deg2rad(-0.6), (-0.02, 0.02, -0.015))]
    windows = [_into_scan_frame(ah.corner(20 + k, 1500), truth[k]) for k in range(3)]
    drifted = [np.eye(4)] * 3                                                    # the pose each window comes with ignores its motion
    plain, reg, rmap = AccumulatedCloud(0.1, DEV, 64), AccumulatedCloud(0.1, DEV, 64), ref.ReferenceMap(0.1)
    for k, pts in enumerate(windows):
        dev_pts = torch.from_numpy(pts).to(DEV)
        plain.add(dev_pts, drifted[k], None, k)
        pose, pose_ref = drifted[k], drifted[k]
        if k:
            res = reg.register(dev_pts, drifted[k], max_iter=MAX_ITER)
            assert int(res['status']) == 0
            pose = res['pose']
            a = _args(dict(init_pose=drifted[k]), MAX_ITER)
            host = _run_host(host_exe, tmp_path, rmap.records(), 0.1, pts, a)
            assert res['pose'].cpu().numpy().tobytes() == host['pose'].tobytes()      # the map so far is the restatement's, record for record
            pose_ref = rref.register(rmap, host['normals32'], host['flags'], pts, drifted[k], max_iter=MAX_ITER)['pose']
            assert _pose_err(pose.cpu().numpy(), truth[k]) < 0.005 < 0.5 * _pose_err(drifted[k], truth[k])      # half the sheets' noise
        reg.add(dev_pts, pose, None, k)
        rmap.add(pts, pose_ref, None, k)
    print('voxels: drifted poses %d, registered %d, restatement %d' % (plain.num_voxels, reg.num_voxels, rmap.num_voxels))
    assert reg.num_voxels < plain.num_voxels
    assert reg.num_voxels <= rmap.num_voxels


@pytest.mark.gpu
def test_argument_errors_and_tables_of_another_filter_gpu():
    from pcaccumulation_amd import native
    m = _device_map('corner')
    pts = torch.from_numpy(_corner_scan()[:100]).to(DEV)
    for bad in (dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=0.1000001), dict(max_distance=float('nan')), dict(max_iter=-1),
                dict(max_iter=10001), dict(radius=0), dict(min_neighbors=2), dict(init_pose=np.eye(3)), dict(moving=torch.zeros(99, device=DEV)),
                dict(viewpoints=np.zeros((4, 2)))):
        with pytest.raises(ValueError):
            m.register(pts, **bad)
    with pytest.raises(ValueError):
        m.register(pts[:, :2])
    with pytest.raises(native.NativeError):
        m.register(pts.cpu())
    with pytest.raises(native.NativeError):
        m.register(pts, moving=torch.zeros(100))
    # normal tables of another filter: values the host knows -- the call says BAD_TABLE, returns init_pose and runs no round
    nrm = m.normals(min_count=3)
    assert 0 < nrm['flags'].shape[0] < m.num_voxels
    init = torch.from_numpy(ah.rot_xyz(0, 0, 0.01, (0.1, 0.2, 0.3))).to(DEV)
    out = native.accum_register(pts, None, init, m.voxel_size, m.voxel_size, 5, m._cur, m.num_voxels, 1, None, nrm['normals'], nrm['flags'])
    assert int(out[4]) == native.REGISTER_BAD_TABLE and torch.equal(out[0], init) and int(out[3]) == 0 and int(out[5]) == 0
    assert float(out[1]) == 0.0 and float(out[2]) == 0.0
    with pytest.raises(native.NativeError):                                      # PCACC_E_ARG: more normal rows than map rows, nothing launched
        native.accum_register(pts, None, None, 0.1, 0.1, 5, m._cur, 10, 1, None, nrm['normals'], nrm['flags'])
    with pytest.raises(native.NativeError):                                      # the gate may not exceed the voxel: the 27 voxels would not cover it
        native.accum_register(pts, None, None, 0.1, 0.2, 5, m._cur, m.num_voxels, 1, None, nrm['normals'], nrm['flags'])


@pytest.mark.gpu
def test_register_results_on_the_model_forward_gpu(golden):
    """register_results on the model_tiny_test forward returns a finite proper rotation.  Nothing more is claimed: its frames are independent random
    clouds."""
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
    flag = out['mos_est'].argmax(1) == 1
    m = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, stamp=0)
    init = ah.rot_xyz(0, 0, 0.01, (0.02, -0.01, 0.0))
    res = m.register_results(out, inp, init_pose=init, max_iter=5)
    same = m.register(out['rec_est'], init, flag, max_iter=5)
    assert all(torch.equal(res[k], same[k]) for k in res)
    pose = res['pose'].cpu().numpy()
    R = pose[:3, :3]
    assert np.all(np.isfinite(pose)) and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0 and np.array_equal(pose[3], [0, 0, 0, 1])
    with pytest.raises(ValueError):
        m.register_results(dict(out, _n_batches=2), inp)
