"""Test-mode clustering (csrc/cluster.hip) on the geometry its invariants exist for; scenes in tests/cluster_scenes.py.

pairs at distance exactly eps and one float32 ulp either side; points with exactly min_samples neighbours; border points in range of two
clusters; voxel coordinates on .5; components thousands of grid cells long; dense cells with border points; +-75 m and 500 m; more kept
voxels than one pass of the launch grid; 64 samples in one call.  Every comparison is exact equality of the int64 label vector.

CPU leg: on every scene, every symmetry of the square, both down-sampling modes and min_p_cluster 1 and 15, the oracle's restated DBSCAN
gives scikit-learn's labels, and the scene still contains what it was built for (its `check`).
GPU leg: the kernel against the oracle (estimator=None; scikit-learn is not needed there), after the same checks."""
import functools

import numpy as np
import pytest
import torch

import cluster_scenes as cs
from pcaccumulation_amd.cluster import Cluster

MIN_P = (1, 15)
SWEPT = ('exact_025', 'exact_05', 'exact_345', 'straddle_04', 'straddle_025', 'shared_border', 'poles', 'ties', 'far', 'samples')
SPIRALS = ('spiral1', 'spiral2')


def _sklearn(eps):
    from sklearn.cluster import DBSCAN
    return DBSCAN(min_samples=cs.MIN_SAMPLES, metric='euclidean', eps=eps)


@functools.lru_cache(None)
def _case(name, sym, use_offset, min_p_cluster):
    """One call's arrays and the oracle's labels for it: computed once, shared by the two legs, read-only."""
    v = cs.variant(cs.scene(name, use_offset, min_p_cluster), sym, use_offset, seed=1 + cs.SYMS.index(sym))
    want = cs.reference(v, min_p_cluster)
    want.setflags(write=False)
    return v, want


def _checked_cases(name, syms):
    """Every (symmetry, mode, min_p_cluster) of a scene, after the scene's own check on the reference result with nothing erased."""
    for sym in syms:
        for use_offset in (True, False):
            for mpc in MIN_P:
                v, want = _case(name, sym, use_offset, mpc)
                if v.scene.name.startswith('samples') or mpc == 1:
                    v.scene.check(v, want)
                yield v, want, mpc


def _run(v, min_p_cluster, fb_labels=None, mos=None, n_batches=None):
    dev = torch.device('cuda:0')
    cfg = {'cluster': {'min_p_cluster': min_p_cluster, 'voxel_size': 0.15, 'min_samples_dbscan': cs.MIN_SAMPLES, 'cluster_metric': 'euclidean',
                       'eps_dbscan': v.eps}}
    n_batches = v.scene.n_batches if n_batches is None else n_batches
    res = {} if n_batches is None else {'_n_batches': n_batches}
    t = lambda a: torch.tensor(a, device=dev)                                # noqa: E731  (a copy: the shared arrays are read-only)
    Cluster(cfg)(t(v.points), t(v.mos if mos is None else mos), t(v.offset), t(v.ti), res,
                 fb_labels=None if fb_labels is None else t(fb_labels), use_offset=v.use_offset)
    return res['inst_labels_est'].cpu().numpy()


def _oracle_is_sklearn(name, syms):
    for v, want, mpc in _checked_cases(name, syms):
        sk = cs.reference(v, mpc, estimator=_sklearn(v.eps))
        assert np.array_equal(want, sk), (name, v.sym, v.use_offset, mpc, int((want != sk).sum()))


def _kernel_is_oracle(name, syms):
    for v, want, mpc in _checked_cases(name, syms):
        got = _run(v, mpc)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, v.sym, v.use_offset, mpc, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ CPU leg
@pytest.mark.parametrize('name', SWEPT)
def test_oracle_is_sklearn(name):
    _oracle_is_sklearn(name, cs.SYMS)


@pytest.mark.parametrize('sym', cs.SYMS, ids=lambda s: ''.join('xyt'[i] for i in range(3) if s[i]) or 'id')
@pytest.mark.parametrize('name', SPIRALS)
def test_oracle_is_sklearn_spiral(name, sym):
    _oracle_is_sklearn(name, [sym])


def test_exact_halves_exist():
    """Scene 6 rests on float32 x with x / float32(voxel) == k + 0.5 exactly: far more than the 50 asked for exist for either voxel size
    (1 206 of the 1 380 k in [20, 70 m / voxel) for 5 cm, 399 of 446 for 15 cm, even and odd k alike)."""
    for voxel in (0.05, 0.15):
        h = cs.exact_halves(voxel, 20, int(70 / voxel))
        assert len(h) >= 50 and sum(k % 2 for k in h) >= 50 and sum(k % 2 == 0 for k in h) >= 50
        for k, x in h.items():
            assert np.float32(x) / np.float32(voxel) == np.float32(k + 0.5)
        assert np.round(np.float32(2.5)) == 2 and cs.round_half_up(np.float32(2.5)) == 3


def test_big_lattice_expectation():
    """The analytic labels of scene 8 against the oracle on a 40 x 30 (and a 33 x 31) instance of the same builder."""
    sc = cs.big_lattices(((40, 30), (33, 31)))
    for use_offset in (True, False):
        v = cs.variant(sc, cs.SYMS[0], use_offset, seed=8)
        for mpc in MIN_P:
            want = cs.reference(v, mpc)
            assert np.array_equal(cs.big_lattice_expected(v), want)
            assert np.array_equal(want, cs.reference(v, mpc, estimator=_sklearn(v.eps)))
        assert (want == 0).sum() == 8


# ------------------------------------------------------------------------------------------------ GPU leg
@pytest.mark.gpu
@pytest.mark.parametrize('name', SWEPT)
def test_cluster_scene_gpu(name):
    _kernel_is_oracle(name, cs.SYMS)


@pytest.mark.gpu
@pytest.mark.parametrize('sym', cs.SYMS, ids=lambda s: ''.join('xyt'[i] for i in range(3) if s[i]) or 'id')
@pytest.mark.parametrize('name', SPIRALS)
def test_cluster_spiral_gpu(name, sym):
    _kernel_is_oracle(name, [sym])


@pytest.mark.gpu
@pytest.mark.parametrize('use_offset', (True, False))
def test_cluster_past_one_grid_pass_gpu(use_offset):
    """560 000 points in 560 000 voxels: more than the 2048 x 256 threads of one pass of the launch grid, in two samples."""
    v = cs.variant(cs.big_lattices(((600, 500), (520, 500))), cs.SYMS[0], use_offset, seed=8)
    assert len(v.mos) == 560000 > 2048 * 256 and v.mos.all()
    want = cs.big_lattice_expected(v)
    assert (want == 0).sum() == 8
    for mpc in MIN_P:
        got = _run(v, mpc)
        assert np.array_equal(got, want), (mpc, int((got != want).sum()))


@pytest.mark.gpu
def test_cluster_sample_limit_gpu():
    """65 samples do not fit the key: an error, not labels."""
    from pcaccumulation_amd import native
    v, _ = _case('samples', cs.SYMS[0], True, 15)
    with pytest.raises(native.NativeError):
        _run(v, 15, n_batches=cs.N_SAMPLES + 1)


@pytest.mark.gpu
def test_cluster_fb_labels_gpu():
    """With fb_labels the selection comes from fb_labels, not from mos."""
    v, want = _case('samples', cs.SYMS[0], True, 15)
    v.scene.check(v, want)
    got = _run(v, 15, fb_labels=v.mos, mos=1 - v.mos)
    assert np.array_equal(got, want)
    inverted = cs.reference(v, 15, mos=1 - v.mos)
    assert not np.array_equal(inverted, want)
    assert np.array_equal(_run(v, 15, mos=1 - v.mos), inverted)
