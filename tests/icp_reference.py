"""Float64 numpy restatement of Open3D's registration_icp with TransformationEstimationPointToPoint, as its documentation states
the algorithm (Open3D itself has no ROCm build and is not a dependency): test infrastructure, never imported by the package.

  correspondences  every source point -> its nearest target point if the distance is within the threshold; brute force, np.argmin,
                   so a tie goes to the lowest target index.  fitness = correspondences / source points,
                   inlier_rmse = sqrt(sum d^2 / correspondences), 0 without correspondences.
  each round       update = least-squares rigid transform of the correspondences (Umeyama without scale: centroids, 3x3 covariance, SVD,
                   reflection fix; identity without correspondences); T = update @ T; the source is transformed by update;
                   correspondences again; stop when |d fitness| < 1e-6 and |d rmse| < 1e-6.
"""
import numpy as np


def nearest(src, tgt, threshold):
    """src [n,3], tgt [m,3] float64 -> (index [n] int64, -1 = none within the threshold; squared distance [n])."""
    n, m = src.shape[0], tgt.shape[0]
    idx = np.full(n, -1, np.int64)
    d2min = np.zeros(n, np.float64)
    if n == 0 or m == 0:
        return idx, d2min
    thr2 = float(threshold) * float(threshold)
    step = max(1, (1 << 22) // m)
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, n, step):
            s = src[lo:lo + step]
            ex = tgt[None, :, 0] - s[:, None, 0]
            ey = tgt[None, :, 1] - s[:, None, 1]
            ez = tgt[None, :, 2] - s[:, None, 2]
            d2 = ex * ex + ey * ey + ez * ez
            d2 = np.where(np.isfinite(d2), d2, np.inf)              # a non-finite coordinate is near nothing
            j = np.argmin(d2, axis=1)                               # first minimum = lowest index
            d = d2[np.arange(s.shape[0]), j]
            ok = d <= thr2
            idx[lo:lo + step] = np.where(ok, j, -1)
            d2min[lo:lo + step] = np.where(ok, d, 0.0)
    return idx, d2min


def evaluate(src, tgt, threshold):
    idx, d2 = nearest(src, tgt, threshold)
    k = int((idx >= 0).sum())
    fitness = k / src.shape[0] if src.shape[0] else 0.0
    rmse = float(np.sqrt(d2.sum() / k)) if k else 0.0
    return idx, fitness, rmse


def umeyama(src, tgt):
    """Least-squares rigid transform taking src [k,3] onto tgt [k,3] (Eigen::umeyama without scaling) as a 4x4."""
    T = np.eye(4)
    if src.shape[0] == 0:
        return T
    ms, mt = src.mean(0), tgt.mean(0)
    cov = (tgt - mt).T @ (src - ms) / src.shape[0]
    U, _, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


def transform(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def rank2_ratio(src, tgt):
    """sigma_1 / sigma_0 of the correspondences' covariance (inf without correspondences: the update is the identity).  At rank >= 2 the rotation
    is determined (the reflection fix settles the third axis); at rank <= 1 -- fewer than three non-collinear correspondences -- the SVD's
    completion of the null space is arbitrary, and with it the answer of ANY implementation, this one included."""
    if src.shape[0] == 0:
        return np.inf
    s = np.linalg.svd((tgt - tgt.mean(0)).T @ (src - src.mean(0)) / src.shape[0], compute_uv=False)
    return float(s[1] / s[0]) if s[0] > 0 else 0.0


def icp(source, target, threshold, init=None, max_iter=50):
    """registration_icp(source.transform(init), target, threshold, eye(4), PointToPoint, max_iteration=max_iter).
    -> dict: T (the registration's transformation), pose (T @ init), fitness, rmse, iterations, correspondences (of the last evaluation),
    rank_ratio (the smallest rank2_ratio any update was computed from)."""
    init = np.eye(4) if init is None else np.asarray(init, np.float64)
    src = transform(init, np.asarray(source, np.float64).reshape(-1, 3))
    tgt = np.asarray(target, np.float64).reshape(-1, 3)
    T = np.eye(4)
    idx, fitness, rmse = evaluate(src, tgt, threshold)
    iterations = 0
    rank_ratio = np.inf
    for _ in range(max_iter):
        sel = idx >= 0
        rank_ratio = min(rank_ratio, rank2_ratio(src[sel], tgt[idx[sel]]))
        update = umeyama(src[sel], tgt[idx[sel]])
        T = update @ T
        src = transform(update, src)
        prev = (fitness, rmse)
        idx, fitness, rmse = evaluate(src, tgt, threshold)
        iterations += 1
        if abs(prev[0] - fitness) < 1e-6 and abs(prev[1] - rmse) < 1e-6:
            break
    return {'T': T, 'pose': T @ init, 'fitness': fitness, 'rmse': rmse, 'iterations': iterations, 'correspondences': idx,
            'rank_ratio': rank_ratio}


def rotation_error_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def rigid(rng, deg, shift):
    """A random rigid motion of about `deg` degrees and `shift` metres."""
    axis = rng.randn(3)
    axis /= np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    d = rng.randn(3)
    T[:3, 3] = shift * d / np.linalg.norm(d)
    return T
