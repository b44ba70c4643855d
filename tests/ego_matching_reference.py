"""Plain-torch restatement of the matching stage of the ego-motion head (pcaccumulation_amd/egomotion.py:22-30 square_distance, :157-166 the padded
log-domain Sinkhorn with slack, :300-312 affinity / exp * support / row sums / soft targets, plus the column sums the outlier loss reads), parameterised
by dtype, for tests/test_ego_matching.py.  float64 gives the expected values and -- through autograd -- the expected gradients; float32 gives the
yardstick: the error the same formulation makes in the kernels' own number format (`bound`).

Also here: the seeded input families of those tests, built so that every discontinuity of the stage (the clamp of the feature distance, the support
threshold) is decided identically in float32 and float64, and the dispatch rule of the Sinkhorn launcher restated (`sinkhorn_paths`)."""
import numpy as np
import torch

EPS = 1e-20                                                                      # toolbox/utils.py:13
DIST_MIN = 1e-12                                                                 # toolbox/utils.py:143
PARAM_POINTS = ((-5.0, -5.0), (-5.0, -5.5), (-1.0, -2.0))                        # the head's initial value; where the clamp defect showed; a warm one


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def square_distance(src, dst, normalised=False):
    dist = -2 * torch.matmul(src, dst.transpose(1, 2))
    if normalised:
        dist = dist + 2
    else:
        dist = dist + torch.sum(src ** 2, dim=-1)[:, :, None] + torch.sum(dst ** 2, dim=-1)[:, None, :]
    return torch.clamp(dist, min=DIST_MIN)


def head_params(alpha, beta):
    """(softplus(alpha), exp(beta) + 0.02) in the dtype of alpha / beta."""
    return torch.nn.functional.softplus(alpha), torch.exp(beta) + 0.02


def affinity(fs, ft, softplus_alpha, denom):
    return -(square_distance(fs, ft, normalised=True) - softplus_alpha) / denom


def sinkhorn(log_alpha, n_iters):
    la = torch.nn.functional.pad(log_alpha, (0, 1, 0, 1))
    for _ in range(n_iters):
        la = torch.cat((la[:, :-1, :] - torch.logsumexp(la[:, :-1, :], dim=2, keepdim=True), la[:, -1, None, :]), dim=1)
        la = torch.cat((la[:, :, :-1] - torch.logsumexp(la[:, :, :-1], dim=1, keepdim=True), la[:, :, -1, None]), dim=2)
    return la[:, :-1, :-1]


def support(cs, ct, thr2):
    return square_distance(cs, ct) < thr2[:, None, None]


def perm_stage(log_perm, cs, ct, thr2):
    """-> (perm [P,k,k], rowsum [P,k,1], weighted_t [P,k,3], colsum [P,k])."""
    perm = torch.exp(log_perm) * support(cs, ct, thr2).to(log_perm.dtype)
    rowsum = torch.sum(perm, dim=2, keepdim=True)
    return perm, rowsum, perm @ ct / (rowsum + EPS), torch.sum(perm, dim=1)


def chain(fs, ft, cs, ct, thr2, alpha, beta, n_iters):
    """Features to perm, all in the dtype of the arguments."""
    a, b = head_params(alpha, beta)
    return perm_stage(sinkhorn(affinity(fs, ft, a, b), n_iters), cs, ct, thr2)[0]


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def errors(kernel, r32, r64):
    """(Ek, E32, floor): max |kernel - R64|, max |R32 - R64| and 2 ulp (float32) of the largest |R64|."""
    r64 = r64.detach().double().cpu()
    ek = float((kernel.detach().double().cpu() - r64).abs().max())
    e32 = float((r32.detach().double().cpu() - r64).abs().max())
    return ek, e32, 2.0 * ulp32(r64.abs().max())


MARGIN = 4.0


def check(name, kernel, r32, r64):
    """Ek <= MARGIN * E32 + floor.  The figures are printed before the assertion (pytest -s shows them)."""
    ek, e32, floor = errors(kernel, r32, r64)
    ratio = ek / e32 if e32 > 0 else (float('inf') if ek > 0 else 0.0)
    line = 'EGO-MATCHING %-44s Ek %.3e  E32 %.3e  floor %.3e  Ek/E32 %.2f' % (name, ek, e32, floor, ratio)
    print(line)
    assert np.isfinite(ek) and ek <= MARGIN * e32 + floor, line


# ---- which kernels a Sinkhorn call runs (csrc/ego.hip, pcacc_sinkhorn_forward / pcacc_sinkhorn_backward) -----------------------------------
def sinkhorn_paths(k, n_iters):
    forward = 'read-only' if k % 4 == 0 else 'in-place'
    backward = 'vector' if k % 4 == 0 and n_iters >= 1 and (2 * n_iters + 1) * k <= (k + 1) ** 2 else 'replay'
    return forward, backward


# ---- input families ------------------------------------------------------------------------------------------------------------------------
def _dyadic_rows(rs, n, c):
    """n rows of exactly four entries +-0.5: unit norm, every dot product a multiple of 0.25 -- exact in float32 in any order, with or without fma."""
    rows = np.zeros((n, c), np.float32)
    for r in rows:
        r[rs.choice(c, 4, replace=False)] = rs.choice((-0.5, 0.5), 4)
    return rows


def dyadic_features(P, k, c, seed=0):
    """-> (fs, ft [P,k,c] float32, identical [P,k,k] bool).  Per pair: k // 2 source rows have their exact copy among the targets (under a random
    permutation); one more target repeats a planted one (a tie); one un-planted source row is the negative of that repeated target (distance 4, the
    affinity minimum, twice).  identical[p,i,j] = rows equal = distance exactly 0 = clamped in every arithmetic; every other distance is >= 0.5."""
    assert c >= 4
    rs = np.random.RandomState(1000 * k + 10 * c + seed)
    fs, ft = np.zeros((P, k, c), np.float32), np.zeros((P, k, c), np.float32)
    for p in range(P):
        fs[p], ft[p] = _dyadic_rows(rs, k, c), _dyadic_rows(rs, k, c)
        m = k // 2
        src, tgt = rs.permutation(k), rs.permutation(k)
        ft[p, tgt[:m]] = fs[p, src[:m]]
        if m >= 1 and k - m >= 1:
            ft[p, tgt[m]] = ft[p, tgt[0]]                                        # k - m >= 1 free targets and sources: always so for k >= 2
            fs[p, src[m]] = -ft[p, tgt[0]]
    identical = (fs[:, :, None, :] == ft[:, None, :, :]).all(-1)
    return torch.from_numpy(fs), torch.from_numpy(ft), torch.from_numpy(identical)


def random_features(P, k, c, seed=0):
    """Normalised Gaussian rows, two thirds of the targets = their source + 0.05 noise, renormalised (as test_sinkhorn_kabsch_full_size_vs_oracle)."""
    rs = np.random.RandomState(2000 * k + 10 * c + seed)
    fs = rs.randn(P, k, c)
    fs /= np.linalg.norm(fs, axis=2, keepdims=True)
    ft = rs.randn(P, k, c)
    m = (2 * k + 2) // 3
    ft[:, :m] = fs[:, :m] + 0.05 * rs.randn(P, m, c)
    ft /= np.linalg.norm(ft, axis=2, keepdims=True)
    return torch.from_numpy(fs.astype(np.float32)), torch.from_numpy(ft.astype(np.float32))


FEATURES = {'dyadic': lambda P, k, c: dyadic_features(P, k, c)[:2], 'random': random_features}

LATTICE_M = 9                                                                    # thr2 of the mixed pair = 9.5


def lattice_coordinates(k, seed=0):
    """-> (cs, ct [3,k,3] float32, thr2 [3] float32).  Integer coordinates, |x| <= 32, thr2 = m + 0.5: squared distances are exact in float32 and
    none sits on a threshold.  Pair 0 is mixed -- source row 0 far from every target (k >= 2: a row without support), source row 1 at squared
    distance exactly m from target 1 and m + 1 from target 2 (k >= 3; at k = 1 the single entry sits at m); pair 1 has no support at all; pair 2
    has full support."""
    rs = np.random.RandomState(3000 + 10 * k + seed)
    cs, ct = np.zeros((3, k, 3), np.float32), np.zeros((3, k, 3), np.float32)
    cs[0], ct[0] = rs.randint(-2, 3, (k, 3)), rs.randint(-2, 3, (k, 3))
    if k == 1:
        cs[0, 0], ct[0, 0] = (1, -2, 0), (1, 1, 0)
    if k >= 2:
        cs[0, 0] = (32, -32, 32)
    if k >= 3:
        cs[0, 1] = (1, -2, 0)
        ct[0, 1] = (1, 1, 0)                                                     # 9 = m: inside
        ct[0, 2] = (2, 1, 0)                                                     # 10 = m + 1: outside
    cs[1], ct[1] = rs.randint(-32, -19, (k, 3)), rs.randint(20, 33, (k, 3))
    cs[2], ct[2] = rs.randint(-1, 2, (k, 3)), rs.randint(-1, 2, (k, 3))          # squared distances <= 12
    thr2 = np.array([LATTICE_M + 0.5, 4.5, 12.5], np.float32)
    return torch.from_numpy(cs), torch.from_numpy(ct), torch.from_numpy(thr2)


def head_affinity(P, k, alpha=-5.0, beta=-5.0):
    """The float64 affinity of the dyadic features (c = 16; 4 at k = 1, 8 below k = 8), rounded to float32: what the Sinkhorn kernels see in the head."""
    c = 4 if k == 1 else (8 if k < 8 else 16)
    fs, ft, _ = dyadic_features(P, k, c)
    a, b = head_params(torch.tensor(alpha, dtype=torch.float64), torch.tensor(beta, dtype=torch.float64))
    return affinity(fs.double(), ft.double(), a, b).float()


def sinkhorn_input(family, P, k):
    """'head': head_affinity at (-5, -5), values in about [-150, 0.3]; 'wide': Gaussian * 40; 'slack': 'head' with two rows and two columns at the
    affinity minimum throughout, so that their mass goes to the slack."""
    if family == 'wide':
        return torch.randn(P, k, k, generator=torch.Generator().manual_seed(7 * P + k)) * 40.0
    x = head_affinity(P, k)
    if family == 'slack':
        a, b = head_params(torch.tensor(-5.0, dtype=torch.float64), torch.tensor(-5.0, dtype=torch.float64))
        low = float((-(4.0 - a) / b).float())
        x[:, :2, :] = low
        x[:, :, -2:] = low
    else:
        assert family == 'head'
    return x
