"""The matching stage in front of the ego pose solve -- ops.ego_affinity, ops.sinkhorn, ops.ego_perm (csrc/ego.hip) and the eval pipeline
native.sinkhorn_kabsch -- against the float64 restatement tests/ego_matching_reference.py, at the temperature the head works at: alpha = beta = -5,
affinities in about [-150, 0.3].

Bounds are not fixed numbers.  With R64 / R32 the restatement in float64 / float32 on the same float32 inputs, every comparison asserts
    Ek = max |kernel - R64|  <=  4 * E32 + floor,    E32 = max |R32 - R64|,    floor = 2 ulp (float32) of the largest |R64|
(gradients: the same, i.e. relative to the largest reference entry).  Exact contracts are asserted exactly: torch.clamp's zero gradient at clamped
feature distances, the support mask, and zero sums / targets / gradients on rows without support.  The input families decide both discontinuities
identically in float32 and float64 (CPU tests below), so no entry has to be excluded.  Measured Ek / E32 per case, and what the tests found: DESIGN.md section 3a."""
import functools

import pytest
import torch

import ego_matching_reference as ref

AFFINITY_SHAPES = ((1, 1, 4), (3, 5, 12), (1, 7, 20), (2, 68, 16), (1, 132, 64))
DYADIC_CHECKED = ((2, 68, 16), (1, 132, 16), (3, 7, 12), (1, 4, 8), (1, 8, 8), (1, 1, 4)) + AFFINITY_SHAPES
# (P, k, iters) -> the forward and the backward form the launcher picks (csrc/ego.hip, pcacc_sinkhorn_forward / _backward)
SINKHORN_CASES = {(2, 1, 3): ('in-place', 'replay'), (2, 7, 0): ('in-place', 'replay'), (1, 8, 0): ('read-only', 'replay'),
                  (2, 4, 3): ('read-only', 'replay'), (1, 8, 5): ('read-only', 'replay'), (2, 8, 3): ('read-only', 'vector'),
                  (1, 12, 5): ('read-only', 'vector'), (2, 68, 3): ('read-only', 'vector'), (1, 132, 5): ('read-only', 'vector'),
                  (2, 65, 3): ('in-place', 'replay'), (1, 129, 2): ('in-place', 'replay')}
PERM_K = (1, 4, 5, 8, 9, 13, 68)
PERM_INPUTS = {'head': (-5.0, -5.0, 5), 'warm': (-1.0, -2.0, 3)}               # (alpha, beta, Sinkhorn iterations) behind the log_perm the stage is fed


def _t64(*ts):
    return [t.double() for t in ts]


def _scalars(alpha, beta, dtype):
    return torch.tensor(alpha, dtype=dtype, requires_grad=True), torch.tensor(beta, dtype=dtype, requires_grad=True)


# ---- CPU: the restatement and the families ---------------------------------------------------------------------------------------------------
def test_restatement_is_the_torch_branch_of_the_head():
    """The float32 restatement against the lines it restates, run from pcaccumulation_amd.egomotion itself: square_distance, the head's softplus and
    parameters, the torch loop of EgoMotionHead.sinkhorn (slack=False selects it; it pads the slack row / column all the same) and lines :307-312."""
    from pcaccumulation_amd import egomotion
    from pcaccumulation_amd.config import default_config
    head = egomotion.EgoMotionHead(default_config('waymo', 'train', n_sweeps=3, xy_range=8))
    assert float(head.alpha) == -5.0 and float(head.beta) == -5.0
    fs, ft = ref.random_features(2, 9, 12)
    cs, ct, thr2 = ref.lattice_coordinates(9)
    cs, ct, thr2 = cs[:2], ct[:2], thr2[:2]
    with torch.no_grad():
        support = (egomotion.square_distance(cs, ct, normalised=False) < thr2[:, None, None]).float()
        affinity = -(egomotion.square_distance(fs, ft, normalised=True) - head.softplus(head.alpha)) / (torch.exp(head.beta) + 0.02)
        perm = torch.exp(head.sinkhorn(affinity, n_iters=3, slack=False)) * support
        rowsum = torch.sum(perm, dim=2, keepdim=True)
        weighted_t = perm @ ct / (rowsum + egomotion._EPS)
        a, b = ref.head_params(head.alpha.detach(), head.beta.detach())
        mine = ref.perm_stage(ref.sinkhorn(ref.affinity(fs, ft, a, b), 3), cs, ct, thr2)
    assert torch.equal(mine[0], perm) and torch.equal(mine[1], rowsum) and torch.equal(mine[2], weighted_t)
    assert torch.equal(mine[3], perm.sum(1)) and 0 < int((perm > 0).sum()) < perm.numel()


@pytest.mark.parametrize('P,k,c', DYADIC_CHECKED)
def test_dyadic_family_clamps_exactly_the_identical_pairs(P, k, c):
    fs, ft, identical = ref.dyadic_features(P, k, c)
    assert torch.equal((fs * fs).sum(2), torch.ones(P, k)) and torch.equal((ft * ft).sum(2), torch.ones(P, k))
    for dt in (torch.float32, torch.float64):
        raw = 2 - 2 * fs.to(dt) @ ft.to(dt).transpose(1, 2)
        assert torch.equal(raw < 1e-12, identical) and torch.equal(raw[identical], torch.zeros(int(identical.sum()), dtype=dt))
        assert bool(identical.all()) or float(raw[~identical].min()) >= 0.5
    assert int(identical.sum()) >= P * (k // 2)
    if k >= 2:
        raw = 2 - 2 * fs @ ft.transpose(1, 2)
        assert all(int((raw[p] == 4).sum()) >= 2 for p in range(P))             # the antipodal source row against the repeated target
        assert all(int(identical[p].sum(1).max()) >= 2 for p in range(P))       # the tie


@pytest.mark.parametrize('P,k,c', AFFINITY_SHAPES)
def test_random_family_stays_off_the_clamp(P, k, c):
    fs, ft = ref.random_features(P, k, c)
    for dt in (torch.float32, torch.float64):
        assert float((2 - 2 * fs.to(dt) @ ft.to(dt).transpose(1, 2)).min()) > 1e-4


@pytest.mark.parametrize('k', PERM_K)
def test_lattice_family_has_the_cases(k):
    cs, ct, thr2 = ref.lattice_coordinates(k)
    assert float(cs.abs().max()) <= 32 and float(ct.abs().max()) <= 32 and torch.equal(cs, cs.round()) and torch.equal(ct, ct.round())
    d2 = ((cs[:, :, None, :].double() - ct[:, None, :, :].double()) ** 2).sum(-1)
    for dt in (torch.float32, torch.float64):
        assert torch.equal(ref.support(cs.to(dt), ct.to(dt), thr2.to(dt)), d2 < thr2.double()[:, None, None])
    mask = d2 < thr2.double()[:, None, None]
    assert not mask[1].any() and mask[2].all()
    assert bool(mask[0].any())
    if k >= 2:
        assert not mask[0, 0].any()                                              # a row without support inside a pair that has some
    if k == 1:
        assert d2[0, 0, 0] == ref.LATTICE_M
    if k >= 3:
        assert d2[0, 1, 1] == ref.LATTICE_M and mask[0, 1, 1] and d2[0, 1, 2] == ref.LATTICE_M + 1 and not mask[0, 1, 2]


def test_sinkhorn_cases_reach_all_four_kernel_pairs():
    for (P, k, iters), listed in SINKHORN_CASES.items():
        assert ref.sinkhorn_paths(k, iters) == listed, (P, k, iters)
    # both forward and both backward implementations, in every pairing the rule allows (the vector backward needs k % 4 == 0: never after in-place)
    assert set(SINKHORN_CASES.values()) == {('in-place', 'replay'), ('read-only', 'replay'), ('read-only', 'vector')}


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from pcaccumulation_amd import native
    native.lib()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _affinity_reference(family, P, k, c, alpha, beta):
    """(inputs, {dtype: (affinity, d fs, d ft, d alpha, d beta)}) of the restatement, computed once per case."""
    fs, ft = ref.FEATURES[family](P, k, c)
    g = torch.randn(P, k, k, generator=torch.Generator().manual_seed(11 * k + c))
    out = {}
    for dt in (torch.float32, torch.float64):
        f1, f2 = fs.to(dt).requires_grad_(True), ft.to(dt).requires_grad_(True)
        al, be = _scalars(alpha, beta, dt)
        aff = ref.affinity(f1, f2, *ref.head_params(al, be))
        out[dt] = [aff.detach()] + [x.detach() for x in torch.autograd.grad((aff * g.to(dt)).sum(), [f1, f2, al, be])]
    return (fs, ft, g), out


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,beta', ref.PARAM_POINTS)
@pytest.mark.parametrize('family', ('dyadic', 'random'))
@pytest.mark.parametrize('P,k,c', AFFINITY_SHAPES)
def test_affinity_forward_backward(dev, P, k, c, family, alpha, beta):
    """Values and the gradients of fs, ft, alpha, beta.  c = 12, 20: the partial channel tile; P k^2 % 4 in {1, 3}: the backward's tail lanes."""
    from pcaccumulation_amd import ops
    (fs, ft, g), r = _affinity_reference(family, P, k, c, alpha, beta)
    f1, f2 = fs.to(dev).requires_grad_(True), ft.to(dev).requires_grad_(True)
    al, be = torch.tensor(alpha, device=dev, requires_grad=True), torch.tensor(beta, device=dev, requires_grad=True)
    aff = ops.ego_affinity(f1, f2, *ref.head_params(al, be))
    grads = torch.autograd.grad((aff * g.to(dev)).sum(), [f1, f2, al, be])
    tag = '%s P%d k%d c%d (%g,%g) ' % (family, P, k, c, alpha, beta)
    for name, got, r32, r64 in zip(('affinity', 'd fs', 'd ft', 'd alpha', 'd beta'), [aff] + list(grads), r[torch.float32], r[torch.float64]):
        ref.check(tag + name, got, r32, r64)


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,beta', ref.PARAM_POINTS)
@pytest.mark.parametrize('P,k,c', AFFINITY_SHAPES)
def test_affinity_backward_blocks_clamped_entries(dev, P, k, c, alpha, beta):
    """torch.clamp's contract, not a tolerance: where the feature distance was clamped (identical rows) d(dot) is exactly 0, elsewhere exactly
    2 g / b; the two scalar gradients do not depend on the clamp."""
    from pcaccumulation_amd import native
    fs, ft, identical = ref.dyadic_features(P, k, c)
    a, b = ref.head_params(torch.tensor(alpha), torch.tensor(beta))
    params = torch.stack([a, b]).to(dev)
    aff = native.ego_affinity_forward(fs.to(dev), ft.to(dev), params)
    g = torch.randn(P, k, k, generator=torch.Generator().manual_seed(k)) + 3.0 * identical.float()    # the matches carry the largest gradients
    grad_dot, grad_params = native.ego_affinity_backward(g.to(dev), aff, params)
    grad_dot, b64 = grad_dot.cpu(), params.double().cpu()[1]
    assert k == 1 or bool(identical.any())
    leaked = (grad_dot != 0) & identical
    assert not leaked.any(), '%d of %d clamped entries received a gradient, largest %g' % (int(leaked.sum()), int(identical.sum()),
                                                                                           float(grad_dot[identical].abs().max()))
    passed = g.double() * (2.0 / b64) * (~identical)
    ref.check('d dot P%d k%d c%d (%g,%g)' % (P, k, c, alpha, beta), grad_dot, passed.float(), passed)
    want = torch.stack([g.double().sum() / b64, -(g.double() * aff.double().cpu()).sum() / b64])
    ref.check('d params P%d k%d c%d (%g,%g)' % (P, k, c, alpha, beta), grad_params, want.float(), want)


@functools.lru_cache(maxsize=None)
def _sinkhorn_reference(family, P, k, iters):
    x = ref.sinkhorn_input(family, P, k)
    gy = torch.randn(P, k, k, generator=torch.Generator().manual_seed(13 * k + iters))
    out = {}
    for dt in (torch.float32, torch.float64):
        xr = x.to(dt).requires_grad_(True)
        y = ref.sinkhorn(xr, iters)
        out[dt] = (y.detach(), torch.exp(y.detach()), torch.autograd.grad((y * gy.to(dt)).sum(), xr)[0])
    return (x, gy), out


@pytest.mark.gpu
@pytest.mark.parametrize('family', ('head', 'wide', 'slack'))
@pytest.mark.parametrize('P,k,iters', sorted(SINKHORN_CASES))
def test_sinkhorn_forward_backward(dev, P, k, iters, family):
    """log_perm, exp(log_perm) and d log_alpha of every kernel pairing, on the head's affinities, on randn * 40 and with rows / columns lost to the slack.

    'wide' is what found the float32 differences of the read-only forward and the vector backward (while x0 - U - V
    was formed in float32 whatever the size of U, exp(log_perm) was 6 - 17 x E32 and the vector backward's d log_alpha 7 - 72 x E32 in the six
    read-only cases with at least one iteration); 'head' and 'slack' keep the largest U below the kernels' float32 / float64 switch, 'wide' is above."""
    from pcaccumulation_amd import ops
    assert ref.sinkhorn_paths(k, iters) == SINKHORN_CASES[(P, k, iters)]       # the kernels this case is here for; revisit the table if the rule moves
    (x, gy), r = _sinkhorn_reference(family, P, k, iters)
    xk = x.to(dev).requires_grad_(True)
    y = ops.sinkhorn(xk, iters)
    gx, = torch.autograd.grad((y * gy.to(dev)).sum(), xk)
    tag = '%s P%d k%d it%d %s/%s ' % ((family, P, k, iters) + SINKHORN_CASES[(P, k, iters)])
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all()), tag
    if iters == 0:
        assert torch.equal(y.cpu(), x) and torch.equal(gx.cpu(), gy), tag        # no normalisation: the input and the gradient come back bit for bit
    missed = []
    for name, got, r32, r64 in zip(('log_perm', 'exp(log_perm)', 'd log_alpha'), (y, torch.exp(y), gx), r[torch.float32], r[torch.float64]):
        # exp(randn * 40) without any normalisation (iters = 0) can exceed float32: there the kernel's value is +inf as the float32 restatement's is
        over = torch.isinf(r32)
        assert torch.equal(torch.isinf(got.detach().cpu()), over) and (iters == 0 or not bool(over.any())), tag + name
        try:
            ref.check(tag + name, got.detach().cpu().masked_fill(over, 0), r32.masked_fill(over, 0), r64.masked_fill(over, 0))
        except AssertionError as e:                                              # all three figures of a case, not only the first that misses
            missed.append(str(e))
    assert not missed, '\n'.join(missed)
    if family == 'slack' and iters >= 1:
        assert float(r[torch.float64][1][:, :2, :].sum(2).max()) < 1e-6          # the minimum rows did lose their mass to the slack


@functools.lru_cache(maxsize=None)
def _perm_reference(which, k):
    """log_perm = the float64 Sinkhorn result of the dyadic features' affinity, rounded to float32; the four results and, per gradient configuration,
    d log_perm of the restatement in both dtypes."""
    alpha, beta, iters = PERM_INPUTS[which]
    lp = ref.sinkhorn(ref.head_affinity(3, k, alpha, beta).double(), iters).float()
    cs, ct, thr2 = ref.lattice_coordinates(k)
    gen = torch.Generator().manual_seed(17 * k)
    gs = [torch.randn(s, generator=gen) for s in ((3, k, k), (3, k, 1), (3, k, 3), (3, k))]
    out = {}
    for dt in (torch.float32, torch.float64):
        x = lp.to(dt).requires_grad_(True)
        res = ref.perm_stage(x, cs.to(dt), ct.to(dt), thr2.to(dt))
        grads = {}
        for cfg in ((0, 1, 2, 3), (0,), (1,), (2,), (3,)):
            grads[cfg] = torch.autograd.grad(sum((res[i] * gs[i].to(dt)).sum() for i in cfg), x, retain_graph=True)[0]
        out[dt] = ([t.detach() for t in res], grads)
    return (lp, cs, ct, thr2, gs), out


@pytest.mark.gpu
@pytest.mark.parametrize('which', sorted(PERM_INPUTS))
@pytest.mark.parametrize('k', PERM_K)
def test_ego_perm_forward_backward(dev, k, which):
    """perm, rowsum, weighted_t, colsum and d log_perm (all four result gradients; each alone: the NULL branches) on lattice coordinates -- rows
    without support, a pair without any, a pair with all of it, entries at m and m + 1 around thr2 = m + 0.5."""
    from pcaccumulation_amd import ops
    (lp, cs, ct, thr2, gs), r = _perm_reference(which, k)
    x = lp.to(dev).requires_grad_(True)
    res = ops.ego_perm(x, cs.to(dev), ct.to(dev), thr2.to(dev))
    (r32, g32), (r64, g64) = r[torch.float32], r[torch.float64]
    tag = '%s k%d ' % (which, k)
    mask = ref.support(cs.double(), ct.double(), thr2.double())
    # the support mask, exactly: zero outside it, and positive inside it wherever float32 can hold exp(log_perm)
    perm, holds = res[0].detach().cpu(), mask & (lp > -80.0)
    assert torch.equal(ref.support(cs, ct, thr2), mask) and torch.equal(r64[0] != 0, mask)
    assert bool((perm[~mask] == 0).all()) and bool((perm[holds] > 0).all()) and (k == 1 or bool(holds[2].any())) and not bool(holds[1].any())
    for i, name in enumerate(('perm', 'rowsum', 'weighted_t', 'colsum')):
        ref.check(tag + name, res[i], r32[i], r64[i])
    dead = ~mask.any(2)                                                          # [3,k] rows without support
    assert bool(dead[1].all()) and not bool(dead[2].any()) and (k < 2 or bool(dead[0, 0]))
    assert torch.equal(res[1].detach().cpu()[dead], torch.zeros(int(dead.sum()), 1))
    assert torch.equal(res[2].detach().cpu()[dead], torch.zeros(int(dead.sum()), 3))
    for cfg in g64:
        gx, = torch.autograd.grad(sum((res[i] * gs[i].to(dev)).sum() for i in cfg), x, retain_graph=True)
        gx = gx.cpu()
        assert bool(torch.isfinite(gx).all()), (tag, cfg)
        assert torch.equal(gx[dead], torch.zeros(int(dead.sum()), k)), (tag, cfg)
        ref.check(tag + 'd log_perm ' + ''.join('prwc'[i] for i in cfg), gx, g32[cfg], g64[cfg])


@pytest.mark.gpu
@pytest.mark.parametrize('P,k,iters', [(2, 68, 3), (1, 132, 5)])
def test_eval_and_training_pipelines_agree_with_float64(dev, P, k, iters):
    """native.sinkhorn_kabsch (eval: the padded in-place kernels) and ego_affinity -> sinkhorn -> ego_perm (training: the read-only kernels) on the
    same dyadic input at the head's temperature: both perm results under the bound of the Sinkhorn test."""
    from pcaccumulation_amd import native, ops
    assert ref.sinkhorn_paths(k, iters)[0] == 'read-only'
    fs, ft, _ = ref.dyadic_features(P, k, 16)
    cs, ct, thr2 = (t[-P:].contiguous() for t in ref.lattice_coordinates(k))     # the last pairs: full support (and none, at P = 2)
    alpha, beta = torch.tensor(-5.0), torch.tensor(-5.0)
    r32 = ref.chain(fs, ft, cs, ct, thr2, alpha, beta, iters)
    r64 = ref.chain(*_t64(fs, ft, cs, ct, thr2, alpha, beta), iters)
    assert float(r64.max()) > 0.3                                                # the planted matches are found (e^0.25 against the slack's e^0 and a tie)
    a, b = ref.head_params(alpha.to(dev), beta.to(dev))
    with torch.no_grad():
        trained = ops.ego_perm(ops.sinkhorn(ops.ego_affinity(fs.to(dev), ft.to(dev), a, b), iters), cs.to(dev), ct.to(dev), thr2.to(dev))[0]
        evaluated, _ = native.sinkhorn_kabsch(fs.to(dev), ft.to(dev), cs.to(dev), ct.to(dev), thr2.to(dev), torch.stack([a, b]).float(), iters)
    ref.check('perm k%d training chain' % k, trained, r32, r64)
    ref.check('perm k%d eval pipeline' % k, evaluated, r32, r64)
