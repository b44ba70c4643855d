"""Float64 restatement of the ego-motion pose solve (toolbox/register_utils.py:263-313, weighted Kabsch with torch.svd) for tests/test_ego_solve.py.
numpy only.  The SVD is LAPACK's: orthonormal factors for every input.

The rotation V diag(1, 1, det(V U^T)) U^T is a function of the matrix alone only where `determinacy` is away from 0; PARITY_CLAIM is where the
tests hold the kernels to this restatement's rotation.  Below it the restatement's own answer is LAPACK's arbitrary choice inside a null space
(or between two nearly tied reflections), and only properties are claimed: orthonormal factors, a proper rotation, the rebuilt matrix, s."""
import numpy as np

PARITY_CLAIM = 1e-3
EPS = 1e-7                                                                       # register_utils.py:247


def svd3_ref(a):
    """a [..., 3, 3] -> (u, s, v) float64 with a = u diag(s) v^T, s descending (torch.svd's convention: v, not v^T)."""
    u, s, vt = np.linalg.svd(np.asarray(a, np.float64))
    return u, s, np.swapaxes(vt, -1, -2)


def rotation_from(u, v):
    """V diag(1, 1, det(V U^T)) U^T (register_utils.py:306-310), float64."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    ut = np.swapaxes(u, -1, -2)
    d = np.ones(u.shape[:-1])
    d[..., 2] = np.linalg.det(v @ ut)
    return (v * d[..., None, :]) @ ut


def rotation_ref(a):
    u, _, v = svd3_ref(a)
    return rotation_from(u, v)


def determinacy(a):
    """(s_1 + d s_2) / s_0, d = sign(det a): how far the rotation is from being undetermined (0 at rank <= 1, and for a reflection whose two
    smallest singular values tie).  0 for the zero matrix."""
    a = np.asarray(a, np.float64)
    s = np.linalg.svd(a, compute_uv=False)
    d = np.sign(np.linalg.det(a))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = (s[..., 1] + d * s[..., 2]) / s[..., 0]
    return np.where(s[..., 0] > 0, r, 0.0)


def kabsch_cov_ref(x1, x2, w):
    """x1, x2 [k,3], w [k] -> (cov [3,3], m1 [3], m2 [3]): register_utils.py:268-293."""
    x1, x2, w = np.asarray(x1, np.float64), np.asarray(x2, np.float64), np.asarray(w, np.float64)
    wn = w / (w.sum() + EPS)
    m1 = (wn[:, None] * x1).sum(0) / (wn.sum() + EPS)
    m2 = (wn[:, None] * x2).sum(0) / (wn.sum() + EPS)
    cov = (x1 - m1).T @ (wn[:, None] * (x2 - m2))
    return cov, m1, m2


def kabsch_ref(x1, x2, w):
    """-> (R [3,3], t [3], cov [3,3]): x2 ~ R x1 + t in the weighted least-squares sense."""
    cov, m1, m2 = kabsch_cov_ref(x1, x2, w)
    R = rotation_ref(cov)
    return R, m2 - R @ m1, cov
