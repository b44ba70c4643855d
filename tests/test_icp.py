"""C3: batched point-to-point ICP (csrc/icp.hip, include/pcacc.h C3) behind model.ego_icp and model.tpointnet_icp.

The reference is tests/icp_reference.py, a float64 numpy restatement of Open3D's documented registration_icp (Open3D has no ROCm build; the
last test of the CPU block compares the restatement with Open3D itself where that is installed).

Order of work.  CPU: csrc/icp_grid.h, icp_round.h and svd3.h -- the code the kernels run -- built with g++ (-ffp-contract=off, every table index
assert-checked): the walk against brute force, then the whole loop against the restatement.  GPU: the kernels against that host build BIT FOR BIT
after one update and at convergence, and against the restatement inside the parity bound below.

Parity bound.  Largest deviation of the kernel from the restatement over the kernel-level scenes of this file (41 jobs), measured on an
MI355X (profiles/icp_parity.txt): pose entries 4.0e-15, translation 3.7e-15 m, angle between the rotations 4.2e-6 degrees (acos next to 1
resolves no better: acos(1 - 2^-53) is 8.5e-7 degrees).  Each bound is ten times its measured maximum, floored at 1e-9, and below the
project's standing 1e-3 degrees / metres: 1e-9 for pose entries, translations and the rmse, 4.2e-5 degrees for the angle.  Fitness is
compared for equality, iteration counts may differ by one.  Covariances of rank <= 1 (fewer than three non-collinear correspondences) are
outside the claim: there the restatement's own answer is LAPACK's arbitrary completion of a null space (tests/icp_reference.py: rank2_ratio).
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import icp_reference as ref
from helpers import build_host_driver
from pcaccumulation_amd.config import default_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_BOUND = 1e-9                    # max(10 * 4.0e-15, 1e-9)
ROT_BOUND_DEG = 4.2e-5               # 10 * 4.2e-6


# ---- scenes (built once, shared, never modified) ---------------------------------------------------------------------------------------
def _moved_subset(rng, tgt, n, deg, shift, outliers=0):
    """n source points: target points pulled back through a small rigid motion (so ICP has that motion to find), fp32; plus far-off outliers."""
    pick = rng.choice(tgt.shape[0], n, replace=tgt.shape[0] < n) if tgt.shape[0] else np.zeros(0, np.int64)
    M = ref.rigid(rng, deg, shift)
    src = ref.transform(np.linalg.inv(M), tgt[pick].astype(np.float64)) if tgt.shape[0] else rng.uniform(-5, 5, (n, 3))
    if outliers:
        src[:outliers] += 3.0
    return src.astype(np.float32)


def _pack(segments, jobs, init=None):
    pts = np.concatenate([s.reshape(-1, 3) for s in segments]).astype(np.float32)
    offsets = np.concatenate(([0], np.cumsum([s.shape[0] for s in segments]))).astype(np.int32)
    jobs = np.asarray(jobs, np.int32).reshape(-1, 2)
    init = np.tile(np.eye(4), (jobs.shape[0], 1, 1)) if init is None else np.asarray(init, np.float64)
    return {'points': pts, 'offsets': offsets, 'jobs': jobs, 'init': init}


def _single_scene():
    rng = np.random.RandomState(0)
    tgt = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    src = _moved_subset(rng, tgt, 256, 2.0, 0.05)
    return dict(_pack([src, tgt], [(0, 1)]), threshold=0.2, max_iter=50)


RAGGED_TARGETS = [0, 1, 300, 500, 800, 1200, 2000, 150]
RAGGED_SOURCES = [40, 60, 0, 1, 2000, 333, 257, 90,       # job j has target j % 8: jobs 0, 8, .. an empty target, jobs 1, 9, .. a one-point target
                  0, 1, 256, 511, 100, 64, 700, 149,       # job 2 and 8: empty source; job 3: one point; job 4: 2000 on 800
                  30, 0, 129, 400, 65, 1000, 77, 31,
                  1, 50, 255, 300, 513, 45, 1999, 120,
                  70, 10, 80, 200, 90, 600, 33, 150]
RAGGED_NOTHING_NEAR = 13                                   # this job's source is moved 50 m away: no point inside the threshold


def _ragged_scene():
    rng = np.random.RandomState(1)
    lo, hi = np.array([-10, -10, -2.0]), np.array([10, 10, 2.0])
    targets = [(lo + rng.uniform(0, 1, (m, 3)) * (hi - lo)).astype(np.float32) for m in RAGGED_TARGETS]
    sources, init = [], []
    for j, n in enumerate(RAGGED_SOURCES):
        s = _moved_subset(rng, targets[j % 8], n, rng.uniform(0.5, 2.0), 0.03, outliers=n // 10)
        if j == RAGGED_NOTHING_NEAR:
            s = s + np.float32(50.0)
        sources.append(s)
        init.append(ref.rigid(rng, 0.3, 0.01) if j % 3 else np.eye(4))          # two thirds of the jobs start from a non-trivial pose
    jobs = [(8 + j, j % 8) for j in range(len(sources))]
    return dict(_pack(targets + sources, jobs, init), threshold=0.2, max_iter=50)


def _tie_scene():
    # a source point midway between two targets that lie in DIFFERENT cells (h = 0.2: x = -0.1 is cell -1, x = +0.1 cell 0): the walk meets the
    # cell of the higher index first in job 1, and must still answer the lowest index.  One correspondence: the update is the translation onto it.
    a = np.array([[-0.1, 0, 0], [0.1, 0, 0]], np.float32)
    b = np.array([[0.1, 0, 0], [-0.1, 0, 0]], np.float32)
    s = np.zeros((1, 3), np.float32)
    return dict(_pack([a, b, s], [(2, 0), (2, 1)]), threshold=0.2, max_iter=50)


def _poisoned(scene, seed=5):
    """The scene with points at 1e9, NaN and Inf mixed into every non-empty segment (source and target side).  Returns (scene, kept mask)."""
    rng = np.random.RandomState(seed)
    bad_rows = np.array([[1e9, 0, 0], [np.nan, 1, 1], [0, np.inf, 0], [2, 2, -np.inf], [-1e9, -1e9, 1e9], [3e38, 0, 0]], np.float32)
    segs, keep = [], []
    for s in range(scene['offsets'].shape[0] - 1):
        seg = scene['points'][scene['offsets'][s]:scene['offsets'][s + 1]]
        if seg.shape[0] == 0:
            segs.append(seg)
            continue
        at = np.sort(rng.randint(0, seg.shape[0] + 1, bad_rows.shape[0]))
        mixed = np.insert(seg, at, bad_rows, axis=0)
        mask = np.insert(np.ones(seg.shape[0], bool), at, False)
        segs.append(mixed)
        keep.append(mask)
    out = dict(_pack(segs, scene['jobs'], scene['init']), threshold=scene['threshold'], max_iter=scene['max_iter'])
    return out, keep


_CACHE = {}


def _scene(name):
    if name not in _CACHE:
        scene = {'single': _single_scene, 'ragged': _ragged_scene, 'tie': _tie_scene}[name]()
        for v in scene.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = scene
    return _CACHE[name]


def _reference(name):
    """The restatement on every job of a scene, computed once."""
    key = name + ':ref'
    if key not in _CACHE:
        sc = _scene(name)
        seg = lambda s: sc['points'][sc['offsets'][s]:sc['offsets'][s + 1]]
        _CACHE[key] = [ref.icp(seg(s), seg(t), sc['threshold'], sc['init'][j], sc['max_iter']) for j, (s, t) in enumerate(sc['jobs'])]
    return _CACHE[key]


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------------
def test_restatement_recovers_known_motion():
    rng = np.random.RandomState(3)
    tgt = rng.uniform(-5, 5, (400, 3))
    M = ref.rigid(rng, 2.0, 0.05)
    src = ref.transform(np.linalg.inv(M), tgt[:300])                            # noise-free, float64
    out = ref.icp(src, tgt, 0.2)
    assert out['fitness'] == 1.0 and out['rmse'] < 1e-12 and 1 <= out['iterations'] < 50
    np.testing.assert_allclose(out['T'], M, atol=1e-12)
    assert np.array_equal(out['correspondences'], np.arange(300))
    # from an initial pose: pose = T @ init is the motion again
    init = ref.rigid(rng, 0.5, 0.02)
    out = ref.icp(ref.transform(np.linalg.inv(init), src), tgt, 0.2, init=init)
    np.testing.assert_allclose(out['pose'], M @ init, atol=1e-12)
    # nothing to match: identity, fitness 0, rmse 0
    for s, t in ((np.zeros((0, 3)), tgt), (src, np.zeros((0, 3))), (src + 100.0, tgt)):
        out = ref.icp(s, t, 0.2)
        assert np.array_equal(out['T'], np.eye(4)) and out['fitness'] == 0.0 and out['rmse'] == 0.0


LOOP_RECORD = np.dtype([('pose', np.float64, (4, 4)), ('fitness', np.float64), ('rmse', np.float64), ('iterations', np.int32), ('status', np.int32)])


def _run_host_driver(exe, tmp_path, sc, tag, max_iter=None):
    """The driver's correspondences under the initial poses; with max_iter, the results of its whole loop instead (one LOOP_RECORD per job)."""
    path, out = str(tmp_path / (tag + '.bin')), str(tmp_path / (tag + '.out'))
    with open(path, 'wb') as f:
        f.write(np.array([sc['points'].shape[0], sc['offsets'].shape[0] - 1, sc['jobs'].shape[0]], np.int64).tobytes())
        f.write(np.array([sc['threshold']], np.float64).tobytes())
        for a, dt in ((sc['points'], np.float32), (sc['offsets'], np.int32), (sc['jobs'], np.int32), (sc['init'], np.float64)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    if max_iter is None:
        subprocess.check_call([exe, path, out])                                 # an assert of the driver aborts it: non-zero exit
        return np.fromfile(out, np.int64)
    loop = str(tmp_path / ('%s.loop%d' % (tag, max_iter)))
    subprocess.check_call([exe, path, out, str(max_iter), loop])
    got = np.fromfile(loop, LOOP_RECORD)
    assert got.shape[0] == sc['jobs'].shape[0]
    return got


def test_host_build_of_the_grid_walk_matches_brute_force(tmp_path):
    """Order of work: the cell / key arithmetic and the 27-cell walk of csrc/icp_grid.h -- the code the kernels run -- compiled with g++, every
    table index assert-checked, on the GPU tests' scenes including the far-away, NaN and Inf points; correspondences = brute force."""
    exe = build_host_driver(tmp_path, 'icp_host_driver')
    poisoned, _ = _poisoned(_scene('ragged'))
    edge = _edge_scene()
    for tag, sc in (('single', _scene('single')), ('ragged', _scene('ragged')), ('tie', _scene('tie')), ('poisoned', poisoned), ('edge', edge)):
        got = _run_host_driver(exe, tmp_path, sc, tag)
        want = []
        for j, (s, t) in enumerate(sc['jobs']):
            with np.errstate(invalid='ignore', over='ignore'):
                src = ref.transform(sc['init'][j], sc['points'][sc['offsets'][s]:sc['offsets'][s + 1]].astype(np.float64))
                tgt = sc['points'][sc['offsets'][t]:sc['offsets'][t + 1]].astype(np.float64)
                # the supported range (include/pcacc.h C3): a point whose cell leaves the key's range has no correspondence, on either side --
                # brute force would pair a source at 1e9 with a target at 1e9
                if True:
                    c = np.floor(src / sc['threshold'])
                    src = np.where(((c >= -32767) & (c <= 32766)).all(1)[:, None], src, np.nan)
                    ct = np.floor(tgt / sc['threshold'])
                    tgt = np.where(((ct >= -32768) & (ct <= 32767)).all(1)[:, None], tgt, np.nan)
            idx, _ = ref.nearest(src, tgt, sc['threshold'])
            want.append(np.where(idx >= 0, idx + sc['offsets'][t], -1))
        want = np.concatenate(want)
        assert got.shape == want.shape, tag
        assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:10])
        if tag in ('single', 'ragged'):
            assert (got >= 0).sum() > 0.5 * got.size                             # the scenes do exercise the walk


def _edge_scene():
    """Points on both sides of the last representable cells (threshold 0.5: cells end at +-16384 m), pairs 0.1 m apart."""
    h = 0.5
    xs = np.array([-32768.5, -32768, -32767.5, -32767, -32766.5, 0, 32765.5, 32766, 32766.5, 32767, 32767.5, 32768, 32768.5]) * h
    tgt = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], 1).astype(np.float32)
    src = (tgt.astype(np.float64) + [0.1, 0, 0]).astype(np.float32)
    sc = _pack([src, tgt, src[:, [1, 0, 2]], tgt[:, [1, 0, 2]], src[:, [1, 2, 0]], tgt[:, [1, 2, 0]]], [(0, 1), (2, 3), (4, 5)])
    return dict(sc, threshold=h, max_iter=5)


def _partition_scene():
    """The smallest scene at which the partition of a source into slices can go wrong: 1603 points and 4 jobs give 7 slices, so job 0 (700 source
    points on 900 targets) is cut into 7 slices of 100 -- every slice ends inside a wave and most lanes of the tree hold 0.0; beside it sources of
    0, 1 and 2 points (fewer points than slices)."""
    rng = np.random.RandomState(11)
    tgt = rng.uniform(-4, 4, (900, 3)).astype(np.float32)
    srcs = [_moved_subset(rng, tgt, n, 1.5, 0.04, outliers=n // 10) for n in (700, 0, 1, 2)]
    return dict(_pack([tgt] + srcs, [(1 + j, 0) for j in range(4)], [ref.rigid(rng, 0.3, 0.01) for _ in range(4)]), threshold=0.2, max_iter=50)


def _reference_in_range(source, target, threshold, init, max_iter):
    """The restatement under the supported range (include/pcacc.h C3): in every evaluation a source point whose cell leaves [-32767, 32766] or a target
    point whose cell leaves [-32768, 32767] has no correspondence -- brute force alone would pair a source beyond the range with a target beyond it."""
    plain = ref.nearest

    def nearest(src, tgt, thr):
        with np.errstate(invalid='ignore', over='ignore'):
            cs, ct = np.floor(src / thr), np.floor(tgt / thr)
            src = np.where(((cs >= -32767) & (cs <= 32766)).all(1)[:, None], src, np.nan)
            tgt = np.where(((ct >= -32768) & (ct <= 32767)).all(1)[:, None], tgt, np.nan)
        return plain(src, tgt, thr)
    ref.nearest = nearest
    try:
        return ref.icp(source, target, threshold, init, max_iter)
    finally:
        ref.nearest = plain


def _loop_scenes():
    """(tag, scene) of everything the whole loop is run on, on the host and on the GPU."""
    if 'loop' not in _CACHE:
        _CACHE['loop'] = (('single', _scene('single')), ('ragged', _scene('ragged')), ('tie', _scene('tie')), ('poisoned', _poisoned(_scene('ragged'))[0]),
                          ('edge', _edge_scene()), ('partition', _partition_scene()))
    return _CACHE['loop']


def test_host_build_of_the_loop_matches_the_restatement(tmp_path):
    """csrc/icp_round.h on csrc/svd3.h -- the slice sums in the kernels' order, the statistics, the stop rule, the status bits, the update and the
    composition the kernels run -- compiled with g++, every index assert-checked, run to the end on every scene: each job against the restatement
    with the bounds the GPU tests apply to the kernel (_assert_job); a job whose covariance is of rank <= 1 in the restatement is outside the claim
    and is held to 'finite proper rotation, status says rank-deficient' for the pose, and to the restatement's fitness, rmse and iterations.  The poisoned scene is held to the clean one as the GPU test holds it."""
    from pcaccumulation_amd import native
    exe = build_host_driver(tmp_path, 'icp_host_driver')
    results = {}
    for tag, sc in _loop_scenes():
        got = _run_host_driver(exe, tmp_path, sc, tag, sc['max_iter'])
        as_gpu = results[tag] = (got['pose'], got['fitness'], got['rmse'], got['iterations'], got['status'])
        n_src = np.diff(sc['offsets'])[sc['jobs'][:, 0]]
        n_tgt = np.diff(sc['offsets'])[sc['jobs'][:, 1]]
        assert np.array_equal((got['status'] & native.ICP_EMPTY_SOURCE) != 0, n_src == 0), tag
        assert np.array_equal((got['status'] & native.ICP_EMPTY_TARGET) != 0, n_tgt == 0), tag
        assert (got['status'] & native.ICP_BAD_TABLE == 0).all(), tag
        if tag == 'poisoned':
            continue
        claimed = deficient = 0
        for j, (s, t) in enumerate(sc['jobs']):
            seg = lambda k: sc['points'][sc['offsets'][k]:sc['offsets'][k + 1]]
            want = _reference(tag)[j] if tag in ('single', 'ragged', 'tie') else _reference_in_range(seg(s), seg(t), sc['threshold'], sc['init'][j], sc['max_iter'])
            _assert_proper_rotation(got['pose'][j])
            matched = want['correspondences'][want['correspondences'] >= 0]
            if want['rank_ratio'] < 1e-6 and np.unique(matched).size >= 2:
                # outside the parity claim for the pose: a null space completed two ways.  (Every source on ONE target is a covariance of zero in exact
                # arithmetic: the identity rotation here -- the noise floor -- and in LAPACK, and the job is compared like any other; the tie scene
                # rests on it.)  The sources of these jobs are collinear -- two points, or the edge scene's rows along an axis -- and the two completions
                # differ by a rotation about their line, which leaves them where they are: fitness, rmse and the stop are the restatement's.
                assert got['status'][j] & native.ICP_RANK_DEFICIENT, (tag, j)
                assert got['fitness'][j] == want['fitness'] and abs(got['rmse'][j] - want['rmse']) <= POSE_BOUND, (tag, j, got['fitness'][j], got['rmse'][j])
                assert abs(int(got['iterations'][j]) - want['iterations']) <= 1, (tag, j)
                deficient += 1
                continue
            _assert_job(tag, j, as_gpu, want)
            claimed += 1
            if want['fitness'] == 0.0:                                          # nothing to match: the pose stays the initial pose
                assert got['status'][j] & native.ICP_NO_CORRESPONDENCE and got['rmse'][j] == 0.0
                np.testing.assert_array_equal(got['pose'][j][:3], sc['init'][j][:3])
        assert deficient == {'partition': 1, 'edge': 3}.get(tag, 0) and claimed + deficient == sc['jobs'].shape[0], (tag, deficient)
    # index 0 of each target segment wins: job 0 moves the source to x = -0.1, job 1 to x = +0.1 (one correspondence: t = mt - ms exactly)
    np.testing.assert_allclose(results['tie'][0][0][:3, 3], [np.float32(-0.1), 0, 0], atol=1e-15)
    np.testing.assert_allclose(results['tie'][0][1][:3, 3], [np.float32(0.1), 0, 0], atol=1e-15)
    _assert_poisoned_equals_clean(_scene('ragged'), dict(_loop_scenes())['poisoned'], results['ragged'], results['poisoned'])


def test_heads_construct_with_icp_flags():
    from pcaccumulation_amd.alignnet import AlignNet
    from pcaccumulation_amd.egomotion import EgoMotionHead
    from pcaccumulation_amd.motionnet import MotionNet
    cfg = default_config('waymo', 'test', n_sweeps=3, xy_range=8)
    assert cfg['model'] == {'ego_icp': False, 'tpointnet_icp': False}           # both off by default
    cfg['model']['ego_icp'] = True
    cfg['model']['tpointnet_icp'] = True
    assert EgoMotionHead(cfg).refine_with_icp is True
    assert AlignNet(cfg).refine_with_icp is True
    model = MotionNet(cfg)
    assert model.ego_motion_head.refine_with_icp and model.reconstructor.refine_with_icp


def test_header_exports_icp_entry_points():
    from pcaccumulation_amd import native
    for name in ('pcacc_icp_point_to_point', 'pcacc_icp_point_to_point_workspace_bytes'):
        assert name in native.EXPORTS
    import ctypes
    args = native._PROTOTYPES['pcacc_icp_point_to_point']
    assert len(args) == 17 and args[7] is ctypes.c_double and args[6] is ctypes.c_void_p
    text = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for word in ('PCACC_ICP_EMPTY_SOURCE 1', 'PCACC_ICP_EMPTY_TARGET 2', 'PCACC_ICP_NO_CORRESPONDENCE 4', 'PCACC_ICP_RANK_DEFICIENT 8',
                 'PCACC_ICP_BAD_TABLE 16'):
        assert word in text
    assert (native.ICP_EMPTY_SOURCE, native.ICP_EMPTY_TARGET, native.ICP_NO_CORRESPONDENCE, native.ICP_RANK_DEFICIENT,
            native.ICP_BAD_TABLE) == (1, 2, 4, 8, 16)


def test_segment_tables_cpu():
    """icp.segments_by_key / anchor_jobs: grouped by key, input order kept inside a segment, negative keys referenced by no segment."""
    from pcaccumulation_amd import icp
    rng = np.random.RandomState(0)
    pts = torch.from_numpy(rng.randn(50, 3).astype(np.float32))
    key = torch.from_numpy(rng.randint(-1, 6, 50))
    grouped, offsets = icp.segments_by_key(pts, key, 6)
    assert offsets.dtype == torch.int32 and offsets.shape == (7,) and int(offsets[0]) == 0
    for k in range(6):
        assert torch.equal(grouped[int(offsets[k]):int(offsets[k + 1])], pts[key == k])
    assert int(offsets[6]) == int((key >= 0).sum())
    assert icp.anchor_jobs(2, 3, torch.device('cpu')).tolist() == [[1, 0], [2, 0], [4, 3], [5, 3]]


def test_restatement_against_open3d():
    o3d = pytest.importorskip('open3d', reason='Open3D is not installed: the restatement of its documented algorithm stands unchecked against it here')
    reg = o3d.pipelines.registration
    for name in ('single', 'ragged', 'tie'):
        sc = _scene(name)
        for j, (s, t) in enumerate(sc['jobs']):
            src = sc['points'][sc['offsets'][s]:sc['offsets'][s + 1]].astype(np.float64)
            tgt = sc['points'][sc['offsets'][t]:sc['offsets'][t + 1]].astype(np.float64)
            if src.shape[0] == 0 or tgt.shape[0] < 3:
                continue
            a, b = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(src)), o3d.geometry.PointCloud(o3d.utility.Vector3dVector(tgt))
            a.transform(sc['init'][j])
            got = reg.registration_icp(a, b, sc['threshold'], np.eye(4), reg.TransformationEstimationPointToPoint(),
                                       reg.ICPConvergenceCriteria(max_iteration=sc['max_iter']))
            want = _reference(name)[j]
            np.testing.assert_allclose(np.array(got.transformation), want['T'], atol=POSE_BOUND)
            assert abs(got.fitness - want['fitness']) < 1e-12 and abs(got.inlier_rmse - want['rmse']) < 1e-9


# ---- GPU tests ----------------------------------------------------------------------------------------------------------------------------
def _run_gpu(sc, dev=None):
    from pcaccumulation_amd import native
    dev = dev or torch.device('cuda:0')
    out = native.icp_point_to_point(torch.from_numpy(np.array(sc['points'])).to(dev), torch.from_numpy(np.array(sc['offsets'])).to(dev),
                                    torch.from_numpy(np.array(sc['jobs'])).to(dev), torch.from_numpy(np.array(sc['init'])).to(dev),
                                    sc['threshold'], sc['max_iter'])
    return [o.cpu().numpy() for o in out]


def _deviation(pose, want):
    return (float(np.abs(pose - want).max()), ref.rotation_error_deg(pose[:3, :3], want[:3, :3]), float(np.linalg.norm(pose[:3, 3] - want[:3, 3])))


def _assert_job(tag, j, got, want):
    pose, fit, rmse, iters, status = got
    dev = _deviation(pose[j], want['pose'])
    print('%s job %d: pose %.3e rot %.3e deg trans %.3e m | fitness %.6f / %.6f iterations %d / %d status %d'
          % (tag, j, dev[0], dev[1], dev[2], fit[j], want['fitness'], iters[j], want['iterations'], status[j]))
    assert np.isfinite(pose[j]).all()
    assert dev[0] <= POSE_BOUND and dev[2] <= POSE_BOUND and dev[1] <= ROT_BOUND_DEG, (tag, j, dev)
    assert fit[j] == want['fitness'], (tag, j)
    assert abs(int(iters[j]) - want['iterations']) <= 1, (tag, j)
    assert abs(rmse[j] - want['rmse']) <= POSE_BOUND, (tag, j)
    return dev


def _assert_proper_rotation(pose, tol=1e-6):
    R = pose[:3, :3]
    assert np.isfinite(pose).all()
    assert abs(np.linalg.det(R) - 1.0) < tol and np.abs(R.T @ R - np.eye(3)).max() < tol
    assert np.array_equal(pose[3], [0, 0, 0, 1])


@pytest.mark.gpu
def test_icp_single_job_gpu():
    sc = _scene('single')
    got = _run_gpu(sc)
    want = _reference('single')[0]
    assert want['fitness'] > 0.9 and want['iterations'] < 50                     # the scene converges
    _assert_job('single', 0, got, want)
    assert got[4][0] == 0


@pytest.mark.gpu
def test_icp_ragged_jobs_gpu():
    from pcaccumulation_amd import native
    sc = _scene('ragged')
    got = _run_gpu(sc)
    wants = _reference('ragged')
    for j, want in enumerate(wants):
        _assert_job('ragged', j, got, want)
        _assert_proper_rotation(got[0][j])
    status = got[4]
    n_src = np.diff(sc['offsets'])[sc['jobs'][:, 0]]
    n_tgt = np.diff(sc['offsets'])[sc['jobs'][:, 1]]
    assert np.array_equal((status & native.ICP_EMPTY_SOURCE) != 0, n_src == 0)
    assert np.array_equal((status & native.ICP_EMPTY_TARGET) != 0, n_tgt == 0)
    assert (status & native.ICP_BAD_TABLE == 0).all()
    for j in np.flatnonzero((n_src == 0) | (n_tgt == 0) | (np.arange(len(wants)) == RAGGED_NOTHING_NEAR)):
        # nothing to match: identity update (the pose stays the initial pose), fitness 0, rmse 0
        assert status[j] & native.ICP_NO_CORRESPONDENCE
        assert got[1][j] == 0.0 and got[2][j] == 0.0
        np.testing.assert_array_equal(got[0][j][:3], sc['init'][j][:3])
    assert (n_src == 1).any() and (n_tgt == 1).any()                             # the single-point jobs are there


@pytest.mark.gpu
def test_icp_tie_goes_to_lowest_index_gpu():
    sc = _scene('tie')
    pose = _run_gpu(sc)[0]
    # index 0 of each target segment wins: job 0 moves the source to x = -0.1, job 1 to x = +0.1
    np.testing.assert_allclose(pose[0][:3, 3], [np.float32(-0.1), 0, 0], atol=1e-15)
    np.testing.assert_allclose(pose[1][:3, 3], [np.float32(0.1), 0, 0], atol=1e-15)
    for j, want in enumerate(_reference('tie')):
        np.testing.assert_allclose(pose[j], want['pose'], atol=POSE_BOUND)


def _assert_poisoned_equals_clean(sc, poisoned, clean, got):
    """clean, got: (pose, fitness, rmse, iterations, status) of the scene and of the scene with far / NaN / Inf points mixed in."""
    n_clean = np.diff(sc['offsets'])[sc['jobs'][:, 0]]
    n_all = np.diff(poisoned['offsets'])[poisoned['jobs'][:, 0]]
    worst = 0.0
    for j in range(sc['jobs'].shape[0]):
        assert np.isfinite(got[0][j]).all()
        dev = _deviation(got[0][j], clean[0][j])
        worst = max(worst, dev[0])
        assert dev[0] <= POSE_BOUND and dev[2] <= POSE_BOUND and dev[1] <= ROT_BOUND_DEG, (j, dev)
        # the same correspondences; the far / NaN / Inf points count in the denominator only
        k_clean, k_all = clean[1][j] * n_clean[j], got[1][j] * n_all[j]
        assert abs(k_clean - k_all) < 1e-6, (j, k_clean, k_all)
        assert abs(got[2][j] - clean[2][j]) <= POSE_BOUND
        assert abs(int(got[3][j]) - int(clean[3][j])) <= 1
    print('poisoned vs clean: largest pose entry deviation %.3e' % worst)
    assert (n_all[n_clean > 0] == n_clean[n_clean > 0] + 6).all()


@pytest.mark.gpu
def test_icp_far_and_non_finite_points_gpu():
    sc = _scene('ragged')
    poisoned, _ = _poisoned(sc)
    _assert_poisoned_equals_clean(sc, poisoned, _run_gpu(sc), _run_gpu(poisoned))


@pytest.mark.gpu
def test_icp_run_to_run_bits_gpu():
    sc = _scene('ragged')
    a, b = _run_gpu(sc), _run_gpu(sc)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_icp_equals_the_host_build_bits_gpu(tmp_path):
    """pcacc_icp_point_to_point against the g++ build of the same headers (icp_grid.h, icp_round.h, svd3.h): pose, fitness, rmse, iterations and
    status BIT FOR BIT, after one update (max_iter = 1) and at convergence, on every scene of the CPU leg -- the partition scene included.  The same
    operations in the same order on IEEE doubles: there is no tolerance to choose."""
    exe = build_host_driver(tmp_path, 'icp_host_driver')
    for tag, sc in _loop_scenes():
        for max_iter in (1, sc['max_iter']):
            host = _run_host_driver(exe, tmp_path, sc, tag, max_iter)
            got = _run_gpu(dict(sc, max_iter=max_iter))
            for name, g in zip(('pose', 'fitness', 'rmse', 'iterations', 'status'), got):
                h = np.ascontiguousarray(host[name])
                assert g.dtype == h.dtype and g.shape == h.shape, (tag, max_iter, name)
                differ = np.flatnonzero((g.reshape(g.shape[0], -1).view(np.uint8) != h.reshape(h.shape[0], -1).view(np.uint8)).any(1))
                assert differ.size == 0, (tag, max_iter, name, differ[:10], g[differ[:2]], h[differ[:2]])
            if max_iter > 1 and tag in ('single', 'ragged', 'partition'):
                assert (got[3] > 1).any() and (got[3] < max_iter).any()          # the loop did iterate, and the stop rule did end it


@pytest.mark.gpu
def test_icp_bad_tables_address_nothing_gpu():
    from pcaccumulation_amd import native
    sc = dict(_scene('single'))
    for offsets, jobs in ((np.array([0, 900, 556], np.int32), sc['jobs']), (sc['offsets'], np.array([[0, 2]], np.int32)),
                          (np.array([0, 256, 10 ** 9], np.int32), sc['jobs']), (sc['offsets'], np.array([[-1, 1]], np.int32))):
        pose, fit, rmse, iters, status = _run_gpu(dict(sc, offsets=offsets, jobs=jobs))
        assert status[0] == native.ICP_BAD_TABLE and np.array_equal(pose[0], np.eye(4)) and fit[0] == 0.0 and iters[0] == 0


def _tiny_model(dev, golden, **flags):
    from helpers import make_batch
    from pcaccumulation_amd.motionnet import MotionNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    g = golden('model_tiny_test')
    cfg = default_config('waymo', 'test', n_sweeps=3, xy_range=8)
    cfg['model'].update(flags)
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
    return cfg, inp, out


def _flag_off(golden):
    if 'model:off' not in _CACHE:
        _CACHE['model:off'] = _tiny_model(torch.device('cuda:0'), golden)
    return _CACHE['model:off']


def _f32_atol(x, ulps):
    """`ulps` fp32 spacings at the largest magnitude of x: the model hands its poses over as fp32."""
    return ulps * float(np.spacing(np.float32(np.abs(x).max())))


@pytest.mark.gpu
def test_model_ego_icp_gpu(golden):
    """model.ego_icp on the model_tiny_test inputs.  Measured on an MI355X: frame 2 starts from 3 correspondences (rank 2) and equals the restatement
    to 1e-15; frame 1 starts from TWO correspondences (fitness 0.0022 of 897 points: the scene's frames are independent random draws, and the
    threshold is 0.1 m) -- a rank-1 covariance, which the issue puts outside the parity claim: there the restatement's own rotation is whatever
    LAPACK makes of a null space (kernel and restatement differ by 4 in pose entries), so that frame is held to 'finite proper rotation, status says
    rank-deficient' instead.  The flag-off forward is not bit-stable run to run on the GPU (2.8e-6 between two runs: atomics in front of the ego
    head), so the initial poses are the refined run's own (`_ego_icp_init`), checked against the flag-off run to the golden tolerance."""
    from pcaccumulation_amd import native
    dev = torch.device('cuda:0')
    g = golden('model_tiny_test')
    cfg, inp, off = _flag_off(golden)
    np.testing.assert_allclose(off['ego_motion_est'].cpu().numpy(), g['ego_motion_est'], atol=1e-3)         # flag off: the golden poses, as before
    assert '_ego_icp_status' not in off and '_ego_icp_init' not in off
    _, _, on = _tiny_model(dev, golden, ego_icp=True)
    est1 = on['ego_motion_est'].cpu().numpy()
    est0 = on['_ego_icp_init'].cpu().numpy().astype(np.float64).reshape(est1.shape)
    np.testing.assert_allclose(est0, off['ego_motion_est'].cpu().numpy(), atol=1e-3)                        # the flag-off poses
    B, T = est0.shape[:2]
    status = on['_ego_icp_status'].cpu().numpy().reshape(B, T - 1)
    pts = inp['input_points'].float().cpu().numpy()
    ti = inp['time_indice'].cpu().numpy().astype(np.int64)
    bg = on['fb_est_per_points'].cpu().numpy()[:, 0] == 0
    pe = cfg['pose_estimation']
    moved, compared = 0.0, 0
    for b in range(B):
        assert np.array_equal(est1[b, 0], np.eye(4, dtype=np.float32))                                      # frame 0 becomes the identity
        tgt = pts[(ti[:, 0] == b) & (ti[:, 1] == 0) & bg]
        for t in range(1, T):
            src = pts[(ti[:, 0] == b) & (ti[:, 1] == t) & bg]
            want = ref.icp(src, tgt, pe['icp_threshold'], est0[b, t], pe['icp_max_iter'])
            print('ego sample %d frame %d: fitness %.6f iterations %d rank ratio %.3e status %d deviation %.3e'
                  % (b, t, want['fitness'], want['iterations'], want['rank_ratio'], status[b, t - 1], np.abs(est1[b, t] - want['pose']).max()))
            _assert_proper_rotation(est1[b, t].astype(np.float64), tol=1e-5)                                # fp32 entries
            if want['rank_ratio'] < 1e-6:                                                                   # outside the parity claim
                assert status[b, t - 1] & native.ICP_RANK_DEFICIENT
                continue
            # the model casts the float64 pose (within POSE_BOUND of the restatement) to fp32 once: one spacing at most on top
            np.testing.assert_allclose(est1[b, t], want['pose'], rtol=0, atol=POSE_BOUND + _f32_atol(want['pose'], 1))
            moved = max(moved, float(np.abs(want['pose'] - est0[b, t]).max()))
            compared += 1
    assert compared >= 1 and moved > 1e-6                                                                   # the refinement did move the poses
    # the errors are formed from the refined poses (egomotion.py:450-458)
    gt = on['ego_motion_gt'].cpu().numpy().astype(np.float64).reshape(-1, 4, 4)
    e1 = est1.astype(np.float64).reshape(-1, 4, 4)
    trans = np.mean([np.linalg.norm(a[:3, 3] - c[:3, 3]) for a, c in zip(e1, gt)]) * T / (T - 1)
    assert abs(on['ego_trans_error'] - trans) < 1e-5


@pytest.mark.gpu
def test_model_tpointnet_icp_gpu(golden):
    """model.tpointnet_icp on the model_tiny_test inputs: every (instance, frame) pose against the restatement run on the package's own fp32
    reconstruction, from the refined run's own pre-refinement estimate (`_inst_icp_init`; the flag-off forward is not bit-stable run to run).
    Jobs whose correspondences are rank <= 1 in the restatement are outside the parity claim (see test_model_ego_icp_gpu) and are held to
    'finite proper rotation, status says rank-deficient'."""
    from pcaccumulation_amd import native
    from pcaccumulation_amd.tpointnet import reconstruct_sequence
    dev = torch.device('cuda:0')
    cfg, inp, off = _flag_off(golden)
    _, _, on = _tiny_model(dev, golden, tpointnet_icp=True)
    assert '_inst_icp_init' not in off and '_icp_anchor_empty' not in off
    pose0 = on['_inst_icp_init']                                                                            # [K,T,4,4] fp32
    K, T = pose0.shape[:2]
    if torch.equal(on['inst_labels_est'], off['inst_labels_est']):                                          # same clusters: the flag-off poses, to the golden tolerance
        np.testing.assert_allclose(pose0.cpu().numpy(), off['inst_pose_est'].cpu().numpy(), rtol=1e-2, atol=1e-2)
    status = on['_inst_icp_status'].cpu().numpy().reshape(K, T - 1)
    rec_idx = on['_rec_idx']
    labels = on['inst_labels_adjusted']
    frames = inp['time_indice'][rec_idx, 1].long()
    pts = on['transformed_points'][rec_idx]
    # AlignNet.padding (alignnet.py:115-163): an instance without frame-0 points gets the points of its first populated frame as frame 0
    lab_np, fr_np = labels.cpu().numpy(), frames.cpu().numpy()
    extra = []
    for k in range(K):
        if not ((lab_np == k) & (fr_np == 0)).any():
            first = fr_np[lab_np == k].min()
            extra.append(np.flatnonzero((lab_np == k) & (fr_np == first)))
    if extra:
        e = torch.from_numpy(np.concatenate(extra)).to(dev)
        pts, labels, frames = torch.cat((pts, pts[e])), torch.cat((labels, labels[e])), torch.cat((frames, torch.zeros_like(e)))
    rec = reconstruct_sequence(pts, frames, labels, pose0, T).cpu().numpy()                                 # the package's own fp32 reconstruction
    lab_np, fr_np = labels.cpu().numpy(), frames.cpu().numpy()
    refined = np.tile(np.eye(4), (K, T, 1, 1))
    claimed = np.ones((K, T), bool)
    for k in range(K):
        tgt = rec[(lab_np == k) & (fr_np == 0)]
        assert tgt.shape[0] > 0
        for t in range(1, T):
            src = rec[(lab_np == k) & (fr_np == t)]
            if src.shape[0]:
                want = ref.icp(src, tgt, cfg['tpointnet']['icp_threshold'], None, 50)
                refined[k, t] = want['T']
                claimed[k, t] = want['rank_ratio'] >= 1e-6
                print('instance %d frame %d: %d on %d points, fitness %.4f iterations %d rank ratio %.3e status %d'
                      % (k, t, src.shape[0], tgt.shape[0], want['fitness'], want['iterations'], want['rank_ratio'], status[k, t - 1]))
    want = torch.matmul(torch.from_numpy(refined.astype(np.float32)).to(dev), pose0).cpu().numpy()          # alignnet.py:110-111, fp32
    got = on['inst_pose_est'].cpu().numpy()
    print('instance poses: %d of %d jobs inside the parity claim, largest deviation there %.3e'
          % (claimed[:, 1:].sum(), claimed[:, 1:].size, np.abs(got - want)[claimed].max()))
    assert claimed[:, 1:].sum() >= 1
    # fp32 product of a refined pose that may sit one fp32 spacing off (a float64 value within POSE_BOUND of the restatement, cast once): four terms
    np.testing.assert_allclose(got[claimed], want[claimed], rtol=0, atol=POSE_BOUND + _f32_atol(want, 8))
    for k, t in zip(*np.nonzero(~claimed)):
        assert status[k, t - 1] & native.ICP_RANK_DEFICIENT
        assert np.isfinite(got[k, t]).all()
    np.testing.assert_array_equal(got[:, 0], pose0[:, 0].cpu().numpy())                                     # frame 0: refined by the identity
    # (on this scene no instance frame has a point within 0.15 m of its anchor frame -- measured: 40 jobs, fitness 0 in every one, kernel and
    # restatement alike -- so the refinement is the identity here; test_refine_instance_poses_gpu moves poses through the same call)
    assert (status & native.ICP_NO_CORRESPONDENCE).any() or np.abs(got - pose0.cpu().numpy()).max() > 0
    assert isinstance(on['inst_l2_error'], float) and np.isfinite(on['inst_l2_error'])                      # the empty-anchor guard let it through


@pytest.mark.gpu
def test_refine_instance_poses_gpu():
    """icp.refine_instance_poses (AlignNet's call) on instances that do overlap: 3 instances x 3 frames, frame t of instance k = its frame-0 points
    under a small motion (at most 9 cm at the far corner: inside the 0.15 m threshold); instance 2 has no points in frame 1 (identity there).  Against the restatement on the package's own reconstruction."""
    from pcaccumulation_amd import icp
    from pcaccumulation_amd.tpointnet import reconstruct_sequence
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(7)
    K, T = 3, 3
    pts, lab, frm = [], [], []
    for k in range(K):
        base = (rng.uniform(-1, 1, (120 + 40 * k, 3)) + [2 * k, 0, 0]).astype(np.float32)
        for t in range(T):
            if k == 2 and t == 1:
                continue
            p = base if t == 0 else _moved_subset(rng, base, 90, 0.3, 0.04)
            pts.append(p); lab.append(np.full(p.shape[0], k)); frm.append(np.full(p.shape[0], t))
    order = rng.permutation(sum(p.shape[0] for p in pts))                                                   # points arrive in no particular order
    pts = torch.from_numpy(np.concatenate(pts)[order]).to(dev)
    lab = torch.from_numpy(np.concatenate(lab)[order]).to(dev)
    frm = torch.from_numpy(np.concatenate(frm)[order]).to(dev)
    pose0 = torch.from_numpy(np.stack([np.stack([ref.rigid(rng, 0.1, 0.01) if t else np.eye(4) for t in range(T)]) for _ in range(K)]).astype(np.float32)).to(dev)
    got, anchor_empty, status = icp.refine_instance_poses(pts, frm, lab, pose0, 0.15, 50)
    assert int(anchor_empty) == 0
    rec = reconstruct_sequence(pts, frm, lab, pose0, T).cpu().numpy()
    l, f = lab.cpu().numpy(), frm.cpu().numpy()
    refined = np.tile(np.eye(4), (K, T, 1, 1))
    for k in range(K):
        for t in range(1, T):
            src = rec[(l == k) & (f == t)]
            if src.shape[0]:
                w = ref.icp(src, rec[(l == k) & (f == 0)], 0.15, None, 50)
                assert w['fitness'] > 0.5 and w['rank_ratio'] > 1e-3                             # the scene does overlap
                refined[k, t] = w['T']
    want = torch.matmul(torch.from_numpy(refined.astype(np.float32)).to(dev), pose0).cpu().numpy()
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=POSE_BOUND + _f32_atol(want, 8))
    assert np.array_equal(got[2, 1].cpu().numpy(), pose0[2, 1].cpu().numpy())                               # a frame without points: identity
    assert np.abs(got.cpu().numpy() - pose0.cpu().numpy()).max() > 1e-3                                     # the poses did move
    # an instance with points but none in frame 0: the flag the host raises on
    keep = ~((lab == 1) & (frm == 0))
    _, anchor_empty, _ = icp.refine_instance_poses(pts[keep], frm[keep], lab[keep], pose0, 0.15, 50)
    assert int(anchor_empty) == 1
