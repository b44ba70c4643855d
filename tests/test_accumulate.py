"""Accumulated scene cloud (include/pcacc.h C4): pcaccumulation_amd.accumulate against the numpy restatement of the
contract, tests/accumulate_reference.py.  The claim is equality -- identical integer records, bit-identical float32 centroids; no tolerance
appears anywhere.

CPU leg: the restatement against a per-point Python loop; csrc/accum_grid.h -- the arithmetic and every index helper the kernels call -- built with
g++ and run stage by stage with every table index assert-checked; the header, the binding and the refusal of CPU tensors.
GPU leg: one add at the sizes where a stage can go wrong, merges at both ends of the map, growth, invalid input, order independence, the extract
filters, save / load, and the model tie-in on the model_tiny_test inputs."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_reference as ref
from accumulate_helpers import DEV
from helpers import ROOT, build_host_driver
from pcaccumulation_amd.config import default_config

FIELDS = ('points', 'coords', 'count', 'moving', 't_first', 't_last')


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _pose(angle, t, axis='z'):
    """Rotation about `axis` by `angle` plus translation t, float64 [4,4]."""
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    i, j = {'x': (1, 2), 'y': (2, 0), 'z': (0, 1)}[axis]
    T[i, i], T[i, j], T[j, i], T[j, j] = c, -s, s, c
    T[:3, 3] = t
    return T


def _cloud(seed, n, lo, hi):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (n, 3)) * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) + np.asarray(lo, np.float64)).astype(np.float32)


def _flags(seed, n, p=0.3):
    return np.random.RandomState(seed).uniform(0, 1, n) < p


def _distinct(n, origin=(0, 0, 0)):
    """n points in n different voxels of edge 1: the centres of a 16 x 16 x k block."""
    i = np.arange(n)
    return (np.stack([i // 256, (i // 16) % 16, i % 16], 1) + 0.5 + np.asarray(origin, np.float64)).astype(np.float32)


# ---- comparison ------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_map(m, r, **extract):
    """Device map m == restatement r: the counters, every integer record, and every field of extract(**extract), bit for bit."""
    assert m.num_voxels == r.num_voxels
    assert m.dropped == r.dropped
    for name, got, want in zip(('keys', 'acc', 'stamps'), m.records(), r.records()):
        assert _same_bits(got, want), name
    got, want = m.extract(**extract), r.extract(**extract)
    assert sorted(got) == sorted(FIELDS)
    for k in FIELDS:
        assert _same_bits(got[k].cpu().numpy(), want[k]), k
    return got


def _add_both(m, r, pts, pose=None, moving=None, stamp=0):
    r.add(pts, pose, moving, stamp)
    m.add(torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), pose, None if moving is None else torch.from_numpy(np.asarray(moving)).to(DEV), stamp)


def _new(voxel_size, capacity=64):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    return AccumulatedCloud(voxel_size, DEV, capacity), ref.ReferenceMap(voxel_size)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------
def test_restatement_unique_formulation_equals_a_per_point_loop():
    pts = _cloud(0, 500, (-3, -3, -1), (3, 3, 1))
    pts[7] = np.nan
    pts[100, 1] = np.inf
    pts[499] = 4e4
    mv = _flags(1, 500)
    a, b = ref.ReferenceMap(0.25), ref.ReferenceMap(0.25)
    for k, (lo, hi) in enumerate(((0, 300), (200, 500))):
        T = _pose(0.3 * k, (0.1, -0.2, 0.05 * k))
        a.add(pts[lo:hi], T, mv[lo:hi], stamp=5 - k)
        b.add_loop(pts[lo:hi], T, mv[lo:hi], stamp=5 - k)
    assert a.dropped == b.dropped == 3
    assert a.num_voxels == b.num_voxels > 100
    for x, y in zip(a.records(), b.records()):
        assert _same_bits(x, y)
    assert max(r[0] for r in a.rec.values()) > 1                                 # some voxel did sum several points


def _run_host_driver(exe, tmp_path, tag, voxel_size, adds, capacity=64, min_count=1, max_moving_fraction=None):
    """adds: [(points, pose or None, moving or None, stamp)] -> the driver's map against the restatement; every assert of the driver aborts it."""
    r = ref.ReferenceMap(voxel_size)
    per_point = []
    chunks = [np.array([len(adds), capacity, min_count, 0 if max_moving_fraction is None else 1], np.int64),
              np.array([0.0 if max_moving_fraction is None else max_moving_fraction, voxel_size], np.float64)]
    for pts, pose, mv, stamp in adds:
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        chunks += [np.array([n, stamp, 0 if pose is None else 1], np.int64), np.ascontiguousarray(np.eye(4) if pose is None else pose, np.float64), pts,
                   np.zeros(n, np.uint8) if mv is None else (np.asarray(mv) != 0).astype(np.uint8)]
        r.add(pts, pose, mv, stamp)
        valid, key, q = ref.per_point(pts, pose, voxel_size)
        per_point.append(np.concatenate([valid[:, None].astype(np.int64), key[:, None], q], 1))
    got = np.frombuffer(ah.run_driver(exe, tmp_path, tag, *chunks, suffix='.bin'), np.int64)
    want_pp = np.concatenate(per_point).reshape(-1)
    assert np.array_equal(got[:want_pp.size], want_pp), (tag, np.flatnonzero(got[:want_pp.size] != want_pp)[:10] // 5)
    got = got[want_pp.size:]
    m, dropped, growths = got[:3]
    keys, acc, stamps = r.records()
    assert (m, dropped) == (r.num_voxels, r.dropped), tag
    got = got[3:]
    assert np.array_equal(got[:m], keys), tag
    assert np.array_equal(got[m:6 * m].reshape(5, m), acc), tag
    assert np.array_equal(got[6 * m:8 * m].reshape(2, m), stamps.astype(np.int64)), tag
    got = got[8 * m:]
    want = r.extract(min_count, max_moving_fraction)
    v = want['count'].shape[0]
    assert got[0] == v and got.size == 1 + 12 * v, tag
    rows = got[1:].reshape(v, 12)
    assert np.array_equal(rows[:, 0:3], want['coords']), tag
    assert np.array_equal(rows[:, 3:6].astype(np.int32), want['points'].view(np.int32)), tag
    for c, k in ((6, 'count'), (7, 'moving'), (8, 't_first'), (9, 't_last')):
        assert np.array_equal(rows[:, c], want[k]), (tag, k)
    return r, int(growths)


def _edge_points(voxel_size):
    """Coordinates that sit on the decisions of the contract, each on every axis in turn (the other two axes at 0.25)."""
    f32 = np.float32
    xs = [f32(k * voxel_size) for k in range(-4, 5)] + [f32(-0.0), f32(0.0)]                     # on voxel boundaries, both signs, -0.0
    for k in (-3, -2, -1, 0, 1, 2, 101, 4096):                                                   # .5 / 65536 ties and their float32 neighbours
        t = f32((k + 0.5) / 65536.0)
        xs += [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))]
    xs += [f32(np.nan), f32(np.inf), f32(-np.inf), f32(32768.0), f32(-32768.0), np.nextafter(f32(32768.0), f32(0)), np.nextafter(f32(-32768.0), f32(0))]
    edge = float(1 << 20) * voxel_size                                                           # the first voxel index outside +-2^20
    for e in (edge, -edge):
        c = f32(e)
        xs += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf)), f32(e * (1 + 2.0 ** -19)), f32(e * (1 - 2.0 ** -19))]
    xs = np.array(xs, np.float32)
    rows = []
    for a in range(3):
        p = np.full((xs.shape[0], 3), 0.25, np.float32)
        p[:, a] = xs
        rows.append(p)
    return np.concatenate(rows)


def test_host_build_of_accum_grid_matches_the_restatement(tmp_path):
    """Order of work: key, validity, fixed point and the reduction / search / merge index helpers of csrc/accum_grid.h -- the code the kernels run --
    compiled with g++, every table index assert-checked, against the restatement, before any GPU test."""
    exe = build_host_driver(tmp_path, 'accum_host_driver')
    for vs in (0.1, 0.01):                                                       # at 0.01 the index bound (+-10485.76) lies inside |w| < 32768
        e = _edge_points(vs)
        r, _ = _run_host_driver(exe, tmp_path, 'edge_%g' % vs, vs, [(e, None, None, 0), (e[::-1], None, _flags(2, e.shape[0]), 1)])
        valid, key, _ = ref.per_point(e, None, vs)
        assert 0 < r.dropped < 2 * e.shape[0] and valid.sum() > 0.5 * e.shape[0]
        if vs == 0.01:                                                           # both sides of the index bound are present
            ix = (key[valid] >> 42) - ref.BIAS
            assert ix.min() == -(1 << 20) and ix.max() == (1 << 20) - 1
            x_only = e[:e.shape[0] // 3, 0].astype(np.float64)
            assert ((np.abs(x_only) < 32768) & ~valid[:e.shape[0] // 3] & np.isfinite(x_only)).sum() >= 4
    # a random 10 k cloud under a rotation + translation pose, then the same region again under another: long runs, hits and misses
    pts = _cloud(3, 10000, (-20, -20, -2), (20, 20, 2))
    adds = [(pts, _pose(0.7, (3.0, -1.5, 0.25)), _flags(4, 10000), 3), (pts[:4000], _pose(-0.2, (0.5, 0.5, 0.0), 'x'), None, 1),
            (_cloud(5, 3000, (-200, 0, 0), (-150, 5, 1)), None, _flags(6, 3000), 2), (_cloud(7, 3000, (150, 0, 0), (200, 5, 1)), None, None, 7),
            (np.zeros((0, 3), np.float32), None, None, 9)]
    r, growths = _run_host_driver(exe, tmp_path, 'random', 0.1, adds, capacity=64, min_count=2, max_moving_fraction=0.25)
    assert r.num_voxels > 10000 and growths >= 8
    # everything in ONE voxel, and every point in its own
    _run_host_driver(exe, tmp_path, 'one', 1.0, [(_cloud(8, 5000, (0.01, 0.01, 0.01), (0.99, 0.99, 0.99)), None, _flags(9, 5000), 0)])
    _run_host_driver(exe, tmp_path, 'distinct', 1.0, [(_distinct(4096), None, None, 0), (_distinct(1000, (4, 0, 0)), None, None, 1)])


def test_header_binding_and_no_cpu_fallback():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud, voxel_mean_downsample
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    names = ('pcacc_accum_add_workspace_bytes', 'pcacc_accum_add', 'pcacc_accum_extract_workspace_bytes', 'pcacc_accum_extract')
    for name in names:
        assert ('int %s(' % name) in header
        assert name in native.EXPORTS
    assert os.path.exists(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_grid.h'))
    assert callable(native.accum_add) and callable(native.accum_extract)
    with pytest.raises(native.NativeError):
        AccumulatedCloud(voxel_size=0.1, device='cuda', capacity=64).add(torch.zeros(4, 3))
    with pytest.raises(native.NativeError):
        voxel_mean_downsample(torch.zeros(4, 3), 0.1)
    with pytest.raises(native.NativeError):
        native.accum_extract((torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32)), 0, 1, None)


def test_one_copy_of_the_launcher_scaffolding():
    """What the launchers of C4 - C11 share is defined once: the wave sum and extract's predicate in accum_launch.h, the three-launch int scan in scan.h.
    A `_scan` that is a __device__ function is not meant (acc_seg_scan of accum.hip is K4's segmented sum over a wave, not a launcher).  voxelize.hip,
    canvas.hip and segment.hip keep their own launches of scan_chunk_sums: the first two pair it with counting kernels of their own."""
    import glob
    import re
    csrc = os.path.join(ROOT, 'pcaccumulation_amd', 'csrc')
    text = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))}
    assert sum(t.count('long long accum_wave_sum(') for t in text.values()) == 1 and 'long long accum_wave_sum(' in text['accum_launch.h']
    for name, t in text.items():
        if name.startswith('accum') and name.endswith('.hip'):
            for line, fn in re.findall(r'^(static [^\n;=]*?\b(\w+)\([^\n;]*)$', t, re.M):
                assert not fn.endswith(('_wave_sum', '_overlap')), (name, fn)
                assert not fn.endswith('_scan') or '__device__' in line, (name, fn)
        if name.startswith('accum') or name in ('icp.hip', 'cluster.hip'):
            assert not re.search(r'scan_chunk_sums|chunk_sums_i32|chunk_scan_i32', t), name
    assert 'hipLaunchKernelGGL(scan_chunk_sums' in text['scan.h'] and 'void pcacc_scan_i32(' in text['scan.h']
    assert not any('accn_keep_kernel' in t for t in text.values())
    assert sum(t.count('void accum_keep_kernel(') for t in text.values()) == 1
    assert open(os.path.join(ROOT, 'pcaccumulation_amd', 'native.py')).read().count('is None else 1') <= 1


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _one_add_case(name):
    if name == 'n1':
        return 0.1, np.array([[1.23, -4.56, 0.78]], np.float32)
    if name == 'n257':
        return 0.1, _cloud(10, 257, (-2, -2, -1), (2, 2, 1))
    if name == 'n2049_block27':
        return 1.0, _cloud(11, 2049, (-1, -1, -1), (2, 2, 2))                    # a 3 x 3 x 3 block of voxels: every run is long
    if name == 'n5000_one_voxel':
        return 1.0, _cloud(12, 5000, (0.01, 0.01, 0.01), (0.99, 0.99, 0.99))     # a run longer than any tile
    assert name == 'n4096_distinct'
    return 1.0, _distinct(4096)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['n1', 'n257', 'n2049_block27', 'n5000_one_voxel', 'n4096_distinct'])
def test_one_add_gpu(case):
    vs, pts = _one_add_case(case)
    n = pts.shape[0]
    m, r = _new(vs, capacity=8192)
    _add_both(m, r, pts, _pose(0.0, (0, 0, 0)) if case == 'n1' else None, _flags(13, n), stamp=4)
    got = _assert_map(m, r)
    assert got['count'].sum().item() == n
    if case == 'n2049_block27':
        assert m.num_voxels == 27
    if case == 'n5000_one_voxel':
        assert m.num_voxels == 1 and got['count'].item() == 5000
    if case == 'n4096_distinct':
        assert m.num_voxels == 4096
    # the same rows from a table that is not 16-byte aligned (the scalar-load leg of the key pass)
    if n > 1:
        m2, r2 = _new(vs, capacity=8192)
        shifted = torch.from_numpy(pts).to(DEV)[1:]
        assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
        m2.add(shifted, stamp=1)
        r2.add(pts[1:], stamp=1)
        _assert_map(m2, r2)


@pytest.mark.gpu
def test_empty_add_is_a_no_op_gpu():
    m, r = _new(0.1)
    m.add(torch.zeros((0, 3), device=DEV))                                       # on an empty map
    assert m.num_voxels == 0 and m.dropped == 0
    assert all(v.shape[0] == 0 for v in m.extract().values())
    _add_both(m, r, _cloud(14, 100, (0, 0, 0), (1, 1, 1)), moving=_flags(15, 100), stamp=2)
    before = [x.copy() for x in m.records()]
    m.add(torch.zeros((0, 3), device=DEV), stamp=9)
    for x, y in zip(before, m.records()):
        assert _same_bits(x, y)
    _assert_map(m, r)


@pytest.mark.gpu
def test_merge_overlap_contained_disjoint_and_both_ends_gpu():
    vs = 0.5
    m, r = _new(vs, capacity=1 << 14)
    rot = lambda a, tx: _pose(a, (tx, 0.3, -0.1), 'x')                           # rotation about x: world x = local x + tx decides the key order
    steps = [('first', _cloud(20, 3000, (0, -4, -1), (10, 4, 1)), rot(0.1, 0.0), 5),
             ('partly overlapping', _cloud(21, 3000, (0, -4, -1), (10, 4, 1)), rot(0.1, 5.0), 3),
             ('fully contained', _cloud(20, 3000, (0, -4, -1), (10, 4, 1))[::7], rot(0.1, 0.0), 8),
             ('every key below', _cloud(22, 2000, (0, -4, -1), (10, 4, 1)), rot(-0.4, -40.0), 1),
             ('every key above', _cloud(23, 2000, (0, -4, -1), (10, 4, 1)), rot(0.9, 60.0), 6)]
    for name, pts, T, stamp in steps:
        lo_before, hi_before, n_before = (min(r.rec), max(r.rec), r.num_voxels) if r.rec else (None, None, 0)
        _, key, _ = ref.per_point(pts, T, vs)
        _add_both(m, r, pts, T, _flags(stamp, pts.shape[0]), stamp)
        _assert_map(m, r)
        new = r.num_voxels - n_before
        uniq = np.unique(key).shape[0]
        if name == 'partly overlapping':
            assert 0 < new < uniq
        if name == 'fully contained':
            assert new == 0
        if name == 'every key below':
            assert key.max() < lo_before and new == uniq
        if name == 'every key above':
            assert key.min() > hi_before and new == uniq
    got = m.extract()
    assert got['t_first'].min().item() == 1 and got['t_last'].max().item() == 8
    assert (got['t_first'] < got['t_last']).any().item()


@pytest.mark.gpu
def test_growth_by_doubling_gpu():
    m, r = _new(1.0, capacity=64)
    caps = []
    for k in range(4):
        _add_both(m, r, _distinct(1000, (4 * k, 0, 0)), stamp=k)                   # 1000 voxels the map does not hold yet
        assert m.num_voxels == r.num_voxels == 1000 * (k + 1)
        caps.append(m.capacity)
        _assert_map(m, r)
    assert caps == [1024, 2048, 4096, 4096]                                      # the tables were re-allocated several times, by doubling


def _poison(pts, vs):
    """Invalid rows of every kind mixed into pts, also as the first and the last row -> (points, mask of the rows that were added)."""
    far_idx = np.float32((1 << 20) * vs * 1.01)                                  # finite, |w| < 32768 at vs = 0.01, voxel index out of range
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [32768, 0, 0], [0, -4e4, 0], [1e30, 1e30, 1e30], [far_idx, 0, 0], [0, 0, -far_idx]],
                   np.float32)
    n = pts.shape[0]
    where = np.concatenate([[0], np.random.RandomState(30).randint(1, n, bad.shape[0] - 2), [n + bad.shape[0] - 1]])
    out = np.insert(pts, np.sort(where[1:-1]), bad[1:-1], axis=0)
    out = np.concatenate([bad[:1], out, bad[-1:]])
    valid, _, _ = ref.per_point(out, None, vs)
    return out, ~valid


@pytest.mark.gpu
def test_invalid_points_are_dropped_and_counted_gpu():
    vs = 0.01
    pts = _cloud(31, 1500, (-3, -3, -1), (3, 3, 1))
    mixed, bad = _poison(pts, vs)
    assert bad.sum() == 8 and bad[0] and bad[-1] and np.array_equal(mixed[~bad], pts)
    mv = _flags(32, mixed.shape[0])
    m, r = _new(vs, capacity=4096)
    _add_both(m, r, mixed, None, mv, stamp=1)
    assert m.dropped == 8
    _assert_map(m, r)
    clean, rc = _new(vs, capacity=4096)
    _add_both(clean, rc, pts, None, mv[~bad], stamp=1)
    for x, y in zip(m.records(), clean.records()):
        assert _same_bits(x, y)                                                  # the valid points give the same map as without the invalid ones
    # an all-invalid call: counted, and the map stays as it is
    _add_both(m, r, mixed[bad], None, None, stamp=2)
    assert m.dropped == 16 and m.num_voxels == clean.num_voxels
    _assert_map(m, r)
    # ... also as the first call on an empty map, and under a pose that throws valid coordinates out of range
    e, re_ = _new(vs)
    _add_both(e, re_, mixed[bad], None, None, stamp=0)
    assert e.num_voxels == 0 and e.dropped == 8
    _add_both(e, re_, pts[:100], _pose(0.0, (32760.0, 0, 0)), None, stamp=0)
    assert e.dropped == 108
    _assert_map(e, re_)


def _run_sequence(adds, vs=0.2):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m = AccumulatedCloud(vs, DEV, 64)
    for pts, T, mv, stamp in adds:
        m.add(torch.from_numpy(pts).to(DEV), T, torch.from_numpy(mv).to(DEV), stamp)
    return m


@pytest.mark.gpu
def test_order_independence_and_reproducibility_gpu(tmp_path):
    a = (_cloud(40, 3000, (-5, -5, -1), (5, 5, 1)), _pose(0.3, (1, 2, 0)), _flags(41, 3000), 2)
    b = (_cloud(42, 2500, (-2, -2, -1), (8, 8, 1)), _pose(-0.5, (0, 0, 0.5)), _flags(43, 2500), 7)
    perm = np.random.RandomState(44).permutation(3000)
    runs = {'base': _run_sequence([a, b]), 'again': _run_sequence([a, b]), 'swapped': _run_sequence([b, a]),
            'permuted': _run_sequence([(a[0][perm], a[1], a[2][perm], a[3]), b])}
    base = runs['base'].extract()
    runs['base'].save(str(tmp_path / 'base.npz'))
    want_bytes = open(str(tmp_path / 'base.npz'), 'rb').read()
    for name in ('again', 'swapped', 'permuted'):
        got = runs[name].extract()
        for k in FIELDS:
            assert torch.equal(got[k], base[k]), (name, k)
        runs[name].save(str(tmp_path / (name + '.npz')))
        assert open(str(tmp_path / (name + '.npz')), 'rb').read() == want_bytes, name
    r = ref.ReferenceMap(0.2)
    for pts, T, mv, stamp in (a, b):
        r.add(pts, T, mv, stamp)
    _assert_map(runs['swapped'], r)


@pytest.mark.gpu
def test_extract_filters_on_the_ratio_gpu():
    vs = 1.0
    centre = lambda x, y, z, k: np.tile(np.array([[x + 0.5, y + 0.5, z + 0.5]], np.float32), (k, 1))
    # (voxel, points, moving): 1 of 4 sits exactly on 0.25; 1 of 3 and 2 of 4 above; 0 of 2 and 0 of 1 below; 4 of 4 all moving
    spec = [((2, 0, 0), 4, 1), ((-1, 3, 0), 3, 1), ((0, 0, 5), 4, 2), ((0, -2, 1), 2, 0), ((-7, 0, 0), 1, 0), ((2, 0, -1), 4, 4), ((0, 0, -5), 8, 2)]
    pts = np.concatenate([centre(*v, k) for v, k, _ in spec])
    mv = np.concatenate([np.arange(k) < j for _, k, j in spec])
    order = np.random.RandomState(50).permutation(pts.shape[0])
    m, r = _new(vs)
    _add_both(m, r, pts[order], None, mv[order], stamp=0)
    assert m.num_voxels == len(spec)
    for kw, kept in ((dict(min_count=1), 7), (dict(min_count=4), 4), (dict(min_count=5), 1), (dict(min_count=9), 0),
                     (dict(max_moving_fraction=0.25), 4), (dict(max_moving_fraction=np.nextafter(0.25, 0)), 2), (dict(max_moving_fraction=0.0), 2),
                     (dict(min_count=3, max_moving_fraction=1.0 / 3.0), 3), (dict(min_count=4, max_moving_fraction=0.25), 2),
                     (dict(max_moving_fraction=1.0), 7)):
        got = _assert_map(m, r, **kw)
        assert got['count'].shape[0] == kept, kw
        c = got['coords'].cpu().numpy().astype(np.int64)
        packed = ((c[:, 0] + ref.BIAS) << 42) | ((c[:, 1] + ref.BIAS) << 21) | (c[:, 2] + ref.BIAS)
        assert np.all(np.diff(packed) > 0), kw                                   # ascending (x, y, z)
    got = m.extract(min_count=4, max_moving_fraction=0.25)
    assert got['coords'].cpu().tolist() == [[0, 0, -5], [2, 0, 0]]


@pytest.mark.gpu
def test_save_load_then_add_equals_the_uninterrupted_sequence_gpu(tmp_path):
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    adds = [(_cloud(60 + k, 2000, (-4 + 2 * k, -4, -1), (4 + 2 * k, 4, 1)), _pose(0.1 * k, (0.5 * k, 0, 0)), _flags(70 + k, 2000), k) for k in range(3)]
    bad = np.full((3, 3), np.nan, np.float32)
    whole, r = _new(0.25)
    part, _ = _new(0.25)
    for k, (pts, T, mv, stamp) in enumerate(adds):
        pts = np.concatenate([pts, bad]) if k == 0 else pts                      # the dropped counter travels with the file
        mv = np.concatenate([mv, np.zeros(3, bool)]) if k == 0 else mv
        _add_both(whole, r, pts, T, mv, stamp)
        if k < 2:
            part.add(torch.from_numpy(pts).to(DEV), T, torch.from_numpy(mv).to(DEV), stamp)
    path = str(tmp_path / 'scene.npz')
    part.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['acc', 'dropped', 'keys', 'stamps', 'voxel_size']
        assert z['keys'].dtype == np.int64 and z['acc'].dtype == np.int64 and z['stamps'].dtype == np.int32
    back = AccumulatedCloud.load(path, DEV)
    assert back.voxel_size == 0.25 and back.num_voxels == part.num_voxels and back.dropped == 3
    for x, y in zip(back.records(), part.records()):
        assert _same_bits(x, y)
    pts, T, mv, stamp = adds[2]
    back.add(torch.from_numpy(pts).to(DEV), T, torch.from_numpy(mv).to(DEV), stamp)
    _assert_map(back, r)
    for x, y in zip(back.records(), whole.records()):
        assert _same_bits(x, y)
    back.clear()
    assert back.num_voxels == 0 and back.dropped == 0 and back.extract()['points'].shape == (0, 3)


@pytest.mark.gpu
def test_voxel_mean_downsample_gpu():
    from pcaccumulation_amd.accumulate import voxel_mean_downsample
    pts = _cloud(80, 3000, (-3, -3, -1), (3, 3, 1))
    got = voxel_mean_downsample(torch.from_numpy(pts).to(DEV), 0.3)
    want = ref.ReferenceMap(0.3).add(pts).extract()['points']
    assert _same_bits(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_model_tie_in_gpu(golden):
    """A test-mode forward on the model_tiny_test inputs: add_results == add(results['rec_est'], moving = the flag the cluster step gets), and the
    static extract holds no voxel that the restatement marks as having a moving point."""
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
        sd['motionhead.offset_head.seg_head.3.weight'] *= float(g['offset_scale'])
        sd['motionhead.offset_head.seg_head.3.bias'] *= float(g['offset_scale'])
        sd['motionhead.mos_seg.seg_head.3.bias'] += torch.tensor([0.0, float(g['mos_shift'])])
    model = model.to(dev).eval().channels_last_()
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
    flag = out['mos_est'].argmax(1) == 1                                         # what MotionNet.forward hands to Cluster, which selects `== 1`
    assert 0 < int(flag.sum()) < flag.shape[0]
    T = _pose(0.4, (2.0, -1.0, 0.1))
    a = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, pose=T, stamp=3)
    b = AccumulatedCloud(0.2, dev, 64).add(out['rec_est'], T, flag, 3)
    for x, y in zip(a.records(), b.records()):
        assert _same_bits(x, y)
    r = ref.ReferenceMap(0.2).add(out['rec_est'].cpu().numpy(), T, flag.cpu().numpy(), 3)
    _assert_map(a, r)
    static = _assert_map(a, r, max_moving_fraction=0.0)
    moving_voxels = {k for k, rec in r.rec.items() if rec[1] > 0}
    assert moving_voxels and len(moving_voxels) < r.num_voxels
    c = static['coords'].cpu().numpy().astype(np.int64)
    kept = set((((c[:, 0] + ref.BIAS) << 42) | ((c[:, 1] + ref.BIAS) << 21) | (c[:, 2] + ref.BIAS)).tolist())
    assert kept and not (kept & moving_voxels)
    assert len(kept) == r.num_voxels - len(moving_voxels)
    with pytest.raises(ValueError):
        a.add_results(dict(out, _n_batches=2), inp, pose=T)                      # two samples need a pose each
