"""The ego-motion pose solve at degenerate and scaled inputs: the 3x3 SVD of pcaccumulation_amd/csrc/svd3.h (called by the fused eval kernel
ego_kabsch_kernel and by the differentiable ops.svd3 of the training path) and the rotation V diag(1, 1, det(V U^T)) U^T built from it, against the
float64 restatement tests/kabsch_reference.py (LAPACK; toolbox/register_utils.py:263-313).

The contract (ego section): u and v are orthonormal and the rotation is proper for EVERY finite input -- rank 2, 1, 0, tiny and huge
matrices included; the rotation equals LAPACK's where kabsch_reference.determinacy >= 1e-3 (the parity claim).  Below that the restatement's own
answer is an arbitrary choice inside a null space and only properties are held.  Which matrices are in the claim is decided by the restatement alone.

CPU leg: svd3.h built with g++ (-ffp-contract=off), float64 outputs, bounds of double arithmetic.
GPU leg: (a) ops.svd3 + ops.kabsch_rt on the same families, fp32 outputs; (b) their gradient against float64 torch.svd + autograd;
(c) the fused kernel through native.sinkhorn_kabsch at k in {3, 7, 65, 257}, healthy and degenerate pairs mixed in one batch, the expected pose
computed from the kernel's own returned perm so that only the Kabsch stage is measured."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import kabsch_reference as ref
from helpers import build_host_driver

POW2 = (-60, -40, -30, -20, 0, 20, 40, 60)
DEC = (1e-18, 1e-12, 1e-10, 1e-9, 1e-6, 1.0, 1e6, 1e12, 1e18)
# families whose every matrix must lie inside the parity claim (asserted from the restatement); the others hold members that are property-only
NEAR_TIES = (1e-2, 1e-4, 1e-6)
ALL_IN_CLAIM = ('scaled_pow2', 'scaled_dec', 'rank2', 'reflect_wide', 'wrong_order') + tuple('near_tie_%.0e' % g for g in NEAR_TIES if g >= 1e-4)
# ... and those with none inside it
NONE_IN_CLAIM = ('rank1_exact', 'rank1_rounded', 'rank0', 'reflect_tight')
ODD_PERMS = ((0, 2, 1), (1, 0, 2), (2, 1, 0))                                 # det = -1 with s_1 = s_2: determinacy 0, the only members of 'ties' outside the claim
RANK1 = ('rank1_exact', 'rank1_rounded')


# ---- matrix families ---------------------------------------------------------------------------------------------------------------------
def _rotations(rs, n):
    q, r = np.linalg.qr(rs.randn(n, 3, 3))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return q


def _sandwich(rs, diag, n):
    """Q1 diag Q2^T under n random rotation pairs."""
    return _rotations(rs, n) @ np.diag(np.asarray(diag, np.float64)) @ np.swapaxes(_rotations(rs, n), 1, 2)


@functools.lru_cache(maxsize=None)
def families():
    """name -> float32 [n,3,3].  What the kernels see IS these float32 values; every expectation is computed from them in float64."""
    rs = np.random.RandomState(20)
    f = {}
    base = rs.randn(64, 3, 3).astype(np.float32)
    f['scaled_pow2'] = np.concatenate([base * np.float32(2.0 ** e) for e in POW2])            # exact: s scales, u / v / R are bit-identical
    f['scaled_dec'] = np.concatenate([base * np.float32(c) for c in DEC])
    x, y, p, q = rs.randn(4, 32, 3)
    f['rank2'] = np.concatenate([x[:, :, None] * y[:, None, :] + p[:, :, None] * q[:, None, :], _sandwich(rs, (3, 2, 0), 32)]).astype(np.float32)
    table = np.zeros((3, 3, 3))
    table[0] = np.outer((1, 2, 3), (1, 2, 3))
    table[1] = 1.0
    table[2, 1, 2] = 5.0
    xq, yq = np.round(rs.randn(2, 29, 3) * 16) / 16                                          # few mantissa bits: x y^T is exact in float32
    xq[:, 0] += (np.abs(xq).sum(1) == 0)
    yq[:, 0] += (np.abs(yq).sum(1) == 0)
    f['rank1_exact'] = np.concatenate([table, xq[:, :, None] * yq[:, None, :]]).astype(np.float32)
    x, y = rs.randn(2, 32, 3)
    f['rank1_rounded'] = (x[:, :, None] * y[:, None, :]).astype(np.float32)                  # rank 1 plus float32 rounding: s_1 ~ 1e-7 s_0
    f['rank0'] = np.zeros((3, 3, 3), np.float32)
    perms = np.stack([np.eye(3)[list(o)] for o in ODD_PERMS + ((0, 1, 2), (1, 2, 0), (2, 0, 1))])
    f['ties'] = np.concatenate([perms] + [c * _rotations(rs, 8) for c in (0.5, 1.0, 3.0)] + [ np.diag((2.0, 2.0, 1.0))[None],
                                                                                  _sandwich(rs, (2, 2, 1), 8)]).astype(np.float32)
    for g in NEAR_TIES:
        f['near_tie_%.0e' % g] = _sandwich(rs, (1 + g, 1, 1 - g), 16).astype(np.float32)
    f['reflect_wide'] = _sandwich(rs, (3, 2, -1), 32).astype(np.float32)                     # det < 0, s_1 - s_2 = s_0 / 3
    f['reflect_tight'] = _sandwich(rs, (3, 1 + 3e-6, -1), 32).astype(np.float32)             # det < 0, s_1 - s_2 = 1e-6 s_0: outside the claim
    wo = np.zeros((6, 3, 3))
    wo[0] = np.diag((1.0, 3.0, 2.0))
    wo[1] = np.diag((2.0, 0.0, 1.0))                                                         # a zero middle column
    wo[2] = np.array([[1.0, 0, 2], [3, 0, 1], [0, 0, 4]])                                    # ... between two columns that do need a rotation
    wo[3] = np.diag((-1.0, 3.0, 2.0))
    wo[4] = np.array([[0.0, 0, 5], [1, 0, 0], [0, 3, 0]])                                    # orthogonal columns, a cyclic shift of the order
    wo[5] = np.array([[1.0, -1, 0], [1, 1, 0], [0, 0, 3]])                                   # orthogonal columns, the last one first, a tie behind it
    f['wrong_order'] = wo.astype(np.float32)
    return f


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement on one family, computed once: (a float64, s_ref, R_ref, in_claim, u0_ref, v0_ref)."""
    a = families()[name].astype(np.float64)
    u, s, v = ref.svd3_ref(a)
    det = ref.determinacy(a)
    out = (a, s, ref.rotation_from(u, v), det >= ref.PARITY_CLAIM, u[:, :, 0], v[:, :, 0])
    for x in out:
        x.setflags(write=False)
    return out


def test_restatement_places_the_families():
    """Which family is in the parity claim follows from the restatement alone, and the restatement is LAPACK's SVD."""
    assert set(ALL_IN_CLAIM + NONE_IN_CLAIM) <= set(families()) and len(ALL_IN_CLAIM) == 7       # a misspelt name must not pass vacuously
    for name in families():
        a, s, R, claim, _, _ = expected(name)
        u, s2, v = ref.svd3_ref(a)
        assert np.abs((u * s2[:, None, :]) @ np.swapaxes(v, 1, 2) - a).max() <= 1e-14 * max(s.max(), 1e-300), name
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(R) - 1).max() <= 1e-14, name
        if name in ALL_IN_CLAIM:
            assert claim.all(), (name, np.flatnonzero(~claim))
        if name in NONE_IN_CLAIM:
            assert not claim.any(), (name, np.flatnonzero(claim))
    # every family is placed: what is left is 'ties' (all but the three odd permutation matrices, its first members) and near_tie_1e-06 (all in)
    assert set(families()) - set(ALL_IN_CLAIM + NONE_IN_CLAIM) == {'ties', 'near_tie_1e-06'}
    assert expected('near_tie_1e-06')[3].all()
    assert np.array_equal(np.flatnonzero(~expected('ties')[3]), np.arange(len(ODD_PERMS))) and len(expected('ties')[3]) == 39
    assert (expected('rank1_exact')[1][:, 1] <= 1e-14 * expected('rank1_exact')[1][:, 0]).all()         # exactly rank 1 as float32 values
    x1 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    c, s_ = np.cos(0.4), np.sin(0.4)
    Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]])
    R, t, _ = ref.kabsch_ref(x1, x1 @ Rz.T + (1.0, 2.0, 3.0), np.ones(4))
    assert np.abs(R - Rz).max() <= 1e-6 and np.abs(t - (1.0, 2.0, 3.0)).max() <= 1e-6       # eps = 1e-7 shrinks the means a little


def _orth(m):
    return np.abs(np.swapaxes(m, -1, -2) @ m - np.eye(3)).reshape(m.shape[0], -1).max(1)


def check_factors(name, u, s, v, orth_tol, rel_tol):
    """Properties that hold for EVERY matrix of a family: u, s, v are float64 arrays holding the outputs under test."""
    a, s_ref, _, _, _, _ = expected(name)
    s0 = s_ref[:, 0]
    print('%s: orth u %.3g v %.3g, rebuild %.3g, s %.3g (relative to s_0)' % (
        name, _orth(u).max(), _orth(v).max(), (np.abs((u * s[:, None, :]) @ np.swapaxes(v, 1, 2) - a).reshape(len(a), -1).max(1) / np.maximum(s0, 1e-300)).max(),
        (np.abs(s - s_ref).max(1) / np.maximum(s0, 1e-300)).max()))
    assert np.isfinite(u).all() and np.isfinite(s).all() and np.isfinite(v).all(), name
    bad = np.flatnonzero(_orth(u) > orth_tol)
    assert bad.size == 0, (name, 'u^T u - I', bad[:8], _orth(u)[bad[:8]])
    bad = np.flatnonzero(_orth(v) > orth_tol)
    assert bad.size == 0, (name, 'v^T v - I', bad[:8], _orth(v)[bad[:8]])
    err = np.abs((u * s[:, None, :]) @ np.swapaxes(v, 1, 2) - a).reshape(len(a), -1).max(1)
    bad = np.flatnonzero(err > rel_tol * s0)
    assert bad.size == 0, (name, 'u diag(s) v^T - a', bad[:8], err[bad[:8]] / s0[bad[:8]])
    assert (s >= 0).all() and (s[:, :-1] >= s[:, 1:]).all(), name
    err = np.abs(s - s_ref).max(1)
    bad = np.flatnonzero(err > rel_tol * s0)
    assert bad.size == 0, (name, 's - s_ref', bad[:8], err[bad[:8]] / s0[bad[:8]])


def check_rotation(name, rot, orth_tol, det_tol, parity_tol):
    """rot float64 [n,3,3]: a proper rotation always; LAPACK's inside the parity claim; at rank 1 it maps u_0 to v_0; the identity at rank 0."""
    _, _, R_ref, claim, u0, v0 = expected(name)
    err = np.abs(rot - R_ref).reshape(len(rot), -1).max(1)
    print('%s: orth rot %.3g, |det - 1| %.3g, |rot - R_ref| in claim %.3g (%d of %d in the claim)' % (
        name, _orth(rot).max(), np.abs(np.linalg.det(rot) - 1).max(), err[claim].max() if claim.any() else 0.0, claim.sum(), len(claim)))
    assert np.isfinite(rot).all(), name
    bad = np.flatnonzero(_orth(rot) > orth_tol)
    assert bad.size == 0, (name, 'rot^T rot - I', bad[:8], _orth(rot)[bad[:8]])
    det = np.abs(np.linalg.det(rot) - 1)
    assert det.max() <= det_tol, (name, 'det', det.max())
    bad = np.flatnonzero(claim & (err > parity_tol))
    assert bad.size == 0, (name, 'rot - R_ref', bad[:8], err[bad[:8]])
    if name in RANK1:                                                            # the one direction the data does determine
        e = np.abs(np.einsum('nij,nj->ni', rot, u0) - v0).max(1)
        assert e.max() <= parity_tol, (name, 'rot u_0 - v_0', e.max())
    if name == 'rank0':
        assert np.array_equal(rot, np.broadcast_to(np.eye(3), rot.shape))


def check_scale_invariance(u, s, v, rot):
    """scaled_pow2: the same 64 matrices times powers of two -- every decision of the routine is relative, so s scales exactly and the rest is bit-identical."""
    n = len(POW2)
    u, s, v, rot = (x.reshape((n, 64) + x.shape[1:]) for x in (u, s, v, rot))
    one = POW2.index(0)
    for i, e in enumerate(POW2):
        assert np.array_equal(u[i], u[one]) and np.array_equal(v[i], v[one]) and np.array_equal(rot[i], rot[one]), e
        assert np.array_equal(s[i], s[one] * s.dtype.type(2.0 ** e)), e


# ---- CPU: svd3.h built on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_svd3(tmp_path_factory):
    d = tmp_path_factory.mktemp('svd3_host')
    exe = build_host_driver(d, 'svd3_host_driver')

    def run(a):
        a = np.ascontiguousarray(a, np.float64).reshape(-1, 9)
        path, out = str(d / 'in.bin'), str(d / 'out.bin')
        with open(path, 'wb') as f:
            f.write(np.array([a.shape[0]], np.int64).tobytes())
            f.write(a.tobytes())
        subprocess.check_call([exe, path, out])
        r = np.fromfile(out, np.float64).reshape(a.shape[0], 21)
        return r[:, :9].reshape(-1, 3, 3), r[:, 9:12].copy(), r[:, 12:].reshape(-1, 3, 3)
    return run


@pytest.mark.parametrize('name', sorted(families()))
def test_svd3_header_on_the_host(host_svd3, name):
    """svd3.h in float64 against LAPACK: factors to 1e-13, the rotation to 1e-9 inside the parity claim (its condition number is
    1 / determinacy <= 1e3, so 1e-9 leaves four digits of slack over 1e-16 * 1e3)."""
    u, s, v = host_svd3(expected(name)[0])
    check_factors(name, u, s, v, orth_tol=1e-13, rel_tol=1e-13)
    rot = ref.rotation_from(u, v)
    check_rotation(name, rot, orth_tol=1e-13, det_tol=1e-13, parity_tol=1e-9)
    if name == 'scaled_pow2':
        check_scale_invariance(u, s, v, rot)
    if name == 'rank0':
        assert np.array_equal(u, np.broadcast_to(np.eye(3), u.shape)) and np.array_equal(v, u) and not s.any()


# ---- GPU (a): ops.svd3 + ops.kabsch_rt -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _means(n, seed=5):
    rs = np.random.RandomState(seed)
    return rs.uniform(-2, 2, (n, 1, 3)).astype(np.float32), rs.uniform(-2, 2, (n, 1, 3)).astype(np.float32)


def _solve(a, m1, m2, dev):
    """float32 numpy in -> float32 numpy (u, s, v, rot, trans) from ops.svd3 + ops.kabsch_rt."""
    from pcaccumulation_amd import ops
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    u, s, v = ops.svd3(t(a))
    rot, trans = ops.kabsch_rt(u, v, t(m1), t(m2))
    assert rot.shape == (a.shape[0], 3, 3) and trans.shape == (a.shape[0], 3, 1)
    return tuple(x.cpu().numpy() for x in (u, s, v, rot, trans[:, :, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(families()))
def test_svd3_and_rotation_on_the_gpu(dev, name):
    """float32 outputs of float64 work.  Orthonormality 1e-6: a 3-term dot product of values rounded to 2^-24 errs by at most ~4e-7.  Rebuild and s
    1e-6 s_0.  |det - 1| 1e-5 and rotation parity 1e-5 (the figure of test_svd3_matches_library_and_its_gradient)."""
    a = families()[name]
    m1, m2 = _means(len(a))
    u, s, v, rot, trans = _solve(a, m1, m2, dev)
    assert all(x.dtype == np.float32 for x in (u, s, v, rot, trans))
    check_factors(name, u.astype(np.float64), s.astype(np.float64), v.astype(np.float64), orth_tol=1e-6, rel_tol=1e-6)
    check_rotation(name, rot.astype(np.float64), orth_tol=1e-6, det_tol=1e-5, parity_tol=1e-5)
    want_t = m2[:, 0].astype(np.float64) - np.einsum('nij,nj->ni', rot.astype(np.float64), m1[:, 0].astype(np.float64))
    # |t| <= 6 rounds to float32 within 2.4e-7; the kernel multiplies its float64 R, this line the rounded one: 3 * 3e-8 * |m1| <= 2e-7 more
    assert np.abs(trans - want_t).max() <= 1e-6
    if name == 'scaled_pow2':
        check_scale_invariance(u, s, v, rot)
    if name == 'rank0':                                                          # LAPACK's answer is the same: rot = I, trans = m2 - m1
        assert np.array_equal(trans, (m2[:, 0].astype(np.float64) - m1[:, 0].astype(np.float64)).astype(np.float32))


@pytest.mark.gpu
def test_host_build_equals_the_kernel_bits(dev, host_svd3):
    """svd3.h switches FMA contraction off and uses only +, -, *, / and sqrt in float64, all correctly rounded on both sides: the factors of the g++
    build, rounded to float32, ARE what ops.svd3 returns, for every matrix of every family.  So the float64 bounds of the CPU leg speak about the
    kernel's own arithmetic."""
    pool = np.concatenate([families()[k] for k in sorted(families())])
    m1, m2 = _means(len(pool))
    u, s, v, _, _ = _solve(pool, m1, m2, dev)
    hu, hs, hv = host_svd3(pool.astype(np.float64))
    for name, got, want in (('u', u, hu), ('s', s, hs), ('v', v, hv)):
        bad = np.flatnonzero((got != want.astype(np.float32)).reshape(len(pool), -1).any(1))
        assert bad.size == 0, (name, bad[:8])


@pytest.mark.gpu
def test_svd3_batch_tails(dev):
    """One lane per matrix, 64 lanes per launch group: batches of 1, 63, 65 and 200 drawn across all families give, row for row, the bits of the
    per-family batches (so every check above holds for them) -- a lane past the end of the batch or one that reads its neighbour's matrix would not."""
    names = sorted(families())
    pool = np.concatenate([families()[k] for k in names])
    m1, m2 = _means(len(pool), seed=6)
    whole = _solve(pool, m1, m2, dev)
    off = 0
    for k in names:                                                              # the pool run IS the per-family runs
        n = len(families()[k])
        part = _solve(pool[off:off + n], m1[off:off + n], m2[off:off + n], dev)
        assert all(np.array_equal(x, y[off:off + n]) for x, y in zip(part, whole)), k
        off += n
    order = np.random.RandomState(7).permutation(len(pool))                      # every batch mixes families, degenerate next to healthy
    for n in (1, 63, 65, 200):
        idx = order[:n]
        got = _solve(pool[idx], m1[idx], m2[idx], dev)
        assert all(x.shape[0] == n and np.array_equal(x, y[idx]) for x, y in zip(got, whole)), n


# ---- GPU (b): the gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pose_gradient_at_separated_singular_values(dev):
    """svd3 -> kabsch_rt -> (R G).sum() + (t g).sum() backward, against float64 torch.svd + autograd on the CPU, at matrices whose relative gaps
    |s_i^2 - s_j^2| / s_0^2 are all >= 1e-2 (chosen from the restatement), unscaled and times 2^-20 and 2^20.  1e-3 of each matrix's largest gradient
    entry: the float32 u, s, v carry ~6e-8, the closed form divides by the gap (<= 100x) and sums O(10) terms -- an order below the bound."""
    from pcaccumulation_amd import ops
    cand = np.random.RandomState(21).randn(256, 3, 3).astype(np.float32)
    cand[0] = np.diag((3.0, 2.0, 1.0))
    cand[1] = -np.abs(cand[1])

    def gaps(a):
        s = ref.svd3_ref(a)[1] ** 2
        return np.minimum(np.minimum(s[:, 0] - s[:, 1], s[:, 1] - s[:, 2]), s[:, 0] - s[:, 2]) / s[:, 0]
    base = cand[gaps(cand) >= 1e-2][:48]
    assert len(base) == 48 and (np.linalg.det(base.astype(np.float64)) < 0).sum() >= 8         # reflections are part of it
    a = np.concatenate([base * np.float32(2.0 ** e) for e in (0, -20, 20)])
    assert (gaps(a) >= 1e-2).all()
    n = len(a)
    m1, m2 = _means(n, seed=8)
    rs = np.random.RandomState(9)
    G, g = rs.randn(n, 3, 3).astype(np.float32), rs.randn(n, 3, 1).astype(np.float32)
    t = lambda x: torch.from_numpy(x)

    ad = t(a).to(dev).requires_grad_(True)
    u, s, v = ops.svd3(ad)
    rot, trans = ops.kabsch_rt(u, v, t(m1).to(dev), t(m2).to(dev))
    ((rot * t(G).to(dev)).sum() + (trans * t(g).to(dev)).sum()).backward()

    ar = t(a).double().requires_grad_(True)
    ur, sr, vr = torch.svd(ar)
    det = torch.det(vr @ ur.transpose(1, 2))
    d = torch.diag_embed(torch.cat((torch.ones((n, 2), dtype=torch.float64), det.unsqueeze(1)), 1))
    rr = vr @ d @ ur.transpose(1, 2)
    tr = t(m2).double().transpose(1, 2) - rr @ t(m1).double().transpose(1, 2)
    ((rr * t(G).double()).sum() + (tr * t(g).double()).sum()).backward()

    assert (rot.detach().cpu().double() - rr.detach()).abs().max().item() <= 1e-5
    scale = ar.grad.abs().amax(dim=(1, 2))
    rel = (ad.grad.cpu().double() - ar.grad).abs().amax(dim=(1, 2)) / scale
    print('gradient: max relative error %.3g (unscaled %.3g, 2^-20 %.3g, 2^20 %.3g)' % (rel.max(), rel[:48].max(), rel[48:96].max(), rel[96:].max()))
    assert torch.isfinite(ad.grad).all() and rel.max().item() <= 1e-3, rel.max().item()


# ---- GPU (c): the fused eval kernel ------------------------------------------------------------------------------------------------------------
SCENES = ('full', 'planar', 'line', 'empty', 'tiny')
TINY = 2.0 ** -16


def _planted():
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(0.2) * K + (1 - np.cos(0.2)) * K @ K, np.array([0.08, -0.03, 0.05])


def _scene(kind, k, c, seed):
    """-> float32 (fs [k,c], ft [k,c], cs [k,3], ct [k,3], thr2).  Target = the planted motion of the source; features match row by row."""
    scale = TINY if kind == 'tiny' else 1.0
    kind = 'full' if kind == 'tiny' else kind
    rs = np.random.RandomState(seed)
    fs = rs.randn(k, c)
    fs /= np.linalg.norm(fs, axis=1, keepdims=True)
    ft = fs + 0.01 * rs.randn(k, c)
    ft /= np.linalg.norm(ft, axis=1, keepdims=True)
    R, tr = _planted()
    while True:                                                                  # a healthy scene is well spread: few points may fall near one line
        cs = np.round(rs.uniform(-1, 1, (k, 3)) * 1024) / 1024
        if kind == 'planar':
            cs[:, 2] = 0.0                                                       # x1 centred has an exactly zero z: rank 2
        if ref.determinacy(ref.kabsch_ref(cs, cs @ R.T + tr, np.ones(k))[2]) >= 0.1:
            break
    if kind == 'line':
        cs = cs[:, :1] * np.array([1.0, 2.0, -0.5])                              # through the origin along a power-of-two direction: the centred
                                                                                 # points stay exact multiples of it, the covariance has rank 1 exactly
    ct = cs @ R.T + tr
    thr2 = 0.0 if kind == 'empty' else 1.0                                       # nothing supported: perm = 0, every weight 0, rank 0
    cs, ct = cs.astype(np.float32) * np.float32(scale), ct.astype(np.float32) * np.float32(scale)      # 'tiny': the float32 scene, scaled exactly;
    thr2 *= scale * scale                                                        # covariance ~ 0.3 * 2^-32 ~ 1e-10
    return tuple(np.ascontiguousarray(x, np.float32) for x in (fs, ft, cs, ct)) + (np.float32(thr2),)


def _run_pairs(native, dev, scenes):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fs, ft, cs, ct, thr2 = (np.stack(x) for x in zip(*scenes))
    params = np.array([np.log1p(np.exp(-5.0)), np.exp(-5.0) + 0.02], np.float32)
    perm, pose = native.sinkhorn_kabsch(t(fs), t(ft), t(cs), t(ct), t(thr2), t(params), 3)
    return perm.cpu().numpy(), pose.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('k', [3, 7, 65, 257])
def test_fused_kernel_pose_at_degenerate_pairs(dev, k):
    """native.sinkhorn_kabsch, P = 4, c = 64, 3 iterations; no k is a multiple of the 256-thread workgroup.  Expected pose = kabsch_ref(cs,
    weighted_t, rowsum) with rowsum and weighted_t formed in float64 from the kernel's own perm.  Rotation 1e-5 and translation
    1e-5 (1 + max |coordinate|) for pairs in the parity claim; the properties of (a) for the others."""
    from pcaccumulation_amd import native
    native.lib()
    c = 64
    scene = {kind: _scene(kind, k, c, 100 * k + (0 if kind == 'tiny' else i)) for i, kind in enumerate(SCENES)}     # 'tiny' is 'full' times 2^-16
    batches = (('full', 'line', 'tiny', 'planar'), ('planar', 'empty', 'full', 'tiny'))        # a degenerate pair between healthy ones
    for kinds in batches:
        perm, pose = _run_pairs(native, dev, [scene[x] for x in kinds])
        assert perm.shape == (4, k, k) and pose.shape == (4, 4, 4) and np.isfinite(pose).all()
        for p, kind in enumerate(kinds):
            _, _, cs, ct, thr2 = scene[kind]
            pm = perm[p].astype(np.float64)
            rowsum = pm.sum(1)
            wt = (pm @ ct.astype(np.float64)) / (rowsum[:, None] + 1e-20)                       # models/egomotion.py:183-184
            R_ref, t_ref, cov = ref.kabsch_ref(cs, wt, rowsum)
            det = float(ref.determinacy(cov))
            rot, tr = pose[p, :3, :3].astype(np.float64), pose[p, :3, 3].astype(np.float64)
            orth, dt = np.abs(rot.T @ rot - np.eye(3)).max(), abs(np.linalg.det(rot) - 1)
            print('k %d %s: sum w %.3g, |cov| %.3g, determinacy %.3g, orth %.3g, |det - 1| %.3g, |rot - R_ref| %.3g, |t - t_ref| %.3g' % (
                k, kind, rowsum.sum(), np.abs(cov).max(), det, orth, dt, np.abs(rot - R_ref).max(), np.abs(tr - t_ref).max()))
            assert np.array_equal(pose[p, 3], np.array([0, 0, 0, 1], np.float32)), kind
            assert orth <= 1e-6 and dt <= 1e-5, (kind, orth, dt)
            if kind == 'empty':
                assert not perm[p].any()
                assert np.array_equal(pose[p], np.eye(4, dtype=np.float32))
                continue
            assert rowsum.sum() > 1e-3 * k, kind                                                # the scene does have supported matches
            if kind == 'tiny':
                assert np.abs(cov).max() <= 1e-9                                                 # inside the range where an absolute stop fails
            if kind == 'line':
                assert det < ref.PARITY_CLAIM
                u, s, v = ref.svd3_ref(cov)
                assert s[1] <= 1e-14 * s[0]                                                      # rank 1 exactly: the completion branch runs
                assert np.abs(rot @ u[:, 0] - v[:, 0]).max() <= 1e-5
                continue
            assert det >= ref.PARITY_CLAIM, (kind, det)                                          # full, planar, tiny: the rotation is determined
            assert np.abs(rot - R_ref).max() <= 1e-5, kind
            assert np.abs(tr - t_ref).max() <= 1e-5 * (1 + max(np.abs(cs).max(), np.abs(ct).max())), kind
        # 'tiny' is 'full' times 2^-16, thr2 times 2^-32: the same support, so the same perm; every coordinate sum scales exactly and every
        # decision of the SVD is relative, so the rotation has the same bits and the translation is the full one times 2^-16
        pf, pt = kinds.index('full'), kinds.index('tiny')
        assert np.array_equal(perm[pt], perm[pf])
        assert np.array_equal(pose[pt, :3, :3], pose[pf, :3, :3]) and np.array_equal(pose[pt, :3, 3], pose[pf, :3, 3] * np.float32(TINY))
        for p, kind in enumerate(kinds):                                                        # a healthy pair does not see its neighbours
            if kind in ('full', 'tiny', 'planar'):
                perm1, pose1 = _run_pairs(native, dev, [scene[kind]])
                assert np.array_equal(perm1[0], perm[p]) and np.array_equal(pose1[0], pose[p]), kind
