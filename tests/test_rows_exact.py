"""The per-point linear layers and the fused PFN block (csrc/mlp.hip, mlp_mfma.hip, mlp_split.hip, pfn_block.hip, pfn_block_split.hip) held to
EXACT integer results at every element.

On small-integer operands every product and partial sum is an integer below 2^24: exact as a bf16 product, as an fp16 hi / lo product of the
power-of-two scaled fp32x3 operands, as an fp32 FMA and in the fp32 MFMA, so summation order, partial slots, atomics and the MFMA layout cannot
change a bit.  The kernel must equal the integer reference of tests/rows_exact_reference.py under torch.equal on the whole tensor; a bf16 value is
the exact value rounded once, to nearest even, at each place include/pcacc.h says a bf16 is held.  There is no tolerance in this file and no
element is excluded: one wrong element, a stale row of the last partial tile, a truncating store, a dropped lo-plane product, a mask predicate that
is wrong at +-0, a gather that reads the neighbouring pooled row, a reduce that skips a slot each change at least one element by at least one unit.

Input families (rows_exact_reference.py): 1 dense small integers; 2 position code (one-hot weights, activations that name their own (piece, row,
column): a mismatch prints where the value came from); 3 fp32x3 lo planes on x and on w separately, one large element fixing the scale, a pooled
piece 2^10 above the point piece, relu(h) needing its lo half inside the PFN block; 4 bf16 mantissa; 5 bf16 output ties, both directions;
6 weights bf16 cannot hold; 7 mask edges {-1, -0.0, +0.0, 2^-126, 1} on every mask and {-1, -0.0, +0.0, 1} under every ReLU (2^-126 times a weight
is no integer and the fp32x3 split flushes it: it is a mask value only).  NaN masks: one rule for every row entry point -- `mask > 0` keeps, NaN
drops -- stated in include/pcacc.h and tested in test_nan_masks_drop_*.

Which kernel variant a shape reaches (PCACC_CUS = 256 workgroup slots; a persistent case has more tiles than the grid)
-------------------------------------------------------------------------------------------------------------------------
bf16 forward, rows_linear_bf16_kernel<K, CT> (CT = n / 32), plain and two-piece: all nine (k, n) in {32, 64, 128}^2, rows in ROWS (tile 128: 1 .. 389 =
partial, full, full + 1, two and three tiles + remainder).  Grid cap = 256 * per_cu, per_cu = min(4, 160 KB / LDS): LDS = 2 (128 (max(k, n) + 8)
+ n (k + 8)) + 4 n bytes gives per_cu 4 for (32, 32), (32, 64), (64, 32), (64, 64), 3 for (32, 128), (64, 128), (128, 32), (128, 64), 2 for
(128, 128): the persistent case of every shape has 128 (256 per_cu) + 129 rows -- the first workgroups take two tiles and prefetch.
fp32x3 forward, rows_linear_split_kernel<K, CT>: the same nine shapes; per_cu = min(3, 160 KB / LDS) -> 3 for (32, 32), (32, 64), (64, 32); 2 for
(64, 64); 1 for every shape with a 128 in it.  rows_linear_split_fm_kernel<128, 4>, <128, 2>, <64, 4> take (128, 128), (128, 64), (64, 128) unless
PCACC_ROWS_FM_OFF is set (grid cap 512): those three shapes run both ways.
bf16 weight gradient, rows_wgrad_bf16_kernel<MAX_TILES, TILE_ROWS, NW>: total = ceil((k + 1) / 32) (n / 32) output tiles; tile rows 256 / 128 / 64 for
k + n <= 64 / <= 128 / above.  (32, 32) <1, 256>; (32, 64), (64, 32) <1, 128>; (64, 64) <2, 128>; (32, 128) <2, 64>; (128, 32), (128, 64)
<2 / 3, 64>; (64, 128) <3, 64>; (128, 128) <3, 64, 8 waves>.  Instantiated and unreachable: <1, 64> (k + n > 128 needs total >= 5).  Grid cap 1024 chunks.
fp32x3 weight gradient, rows_wgrad_split_kernel: tile rows 128 for k, n <= 64, else 64; <1, 128> (32, 32), (32, 64), (64, 32); <2, 128> (64, 64);
<2, 64> (32, 128), (128, 32); <3, 64> (64, 128), (128, 64); <3, 64, 8> (128, 128).  <1, 64> unreachable as above.  Grid cap <= 768 chunks.
fp32 kernels (mlp.hip): rows_linear_kernel<K, 128> for max(k, n) <= 64, <K, 64> above, every K in {2, 3, 4, 9, 32, 64, 128} with n in {3, 7, 33, 100,
128} (k <= 9 with n = 128 is the few-input kernel; grid cap 4096 tiles); rows_linear_fewk_kernel<K, n / 8, HALVES>: HALVES = true with an fp32 y,
false with a bf16 y; rows_linear_few_dual = the HALVES form with y16 / y_amax; rows_linear_fewn_kernel<K, 1 | 2>; rows_wgrad_kernel<ROWS, T>: <96, 1>
(32, 32), <96, 2> (64, 48), <32, 1> (16, 128), <32, 2> (64, 64), <32, 6> (128, 128) -- <96, 6> is instantiated and unreachable (more than 8 output
tiles need k + n > 120); rows_wgrad_few_kernel<F, C / 4, FAST>: FAST 1 / 2 = few inputs with bf16 dY (and bf16 mask) and fp32 X, 0 otherwise.
PFN block: pfn_block_fwd / bwd_kernel<GATHER>, pfn_block_split_fwd / dgrad_kernel, grid caps 768 / 512 / 512 / 512 tiles of 128 rows: rows in
PFN_ROWS and one case of 768 * 128 + 129 rows.
Autograd paths: ops.linear_rows, ResnetBlockFC.forward_pooled and ops.pfn_block(pool=True) in the bf16, fp32x3 and mixed modes at 2048 + 129 rows (the
fused kernels start at 2048): output, data, weight and bias gradients, the pooled rows' gradient (fp32 per-pillar sums, stored once in the rows' type).

Order-dependent contracts: none was found.  Every case below is exact; the cap on excluded elements is zero."""
import functools

import pytest
import torch

import rows_exact_reference as R
from pcaccumulation_amd import native, ops

gpu = pytest.mark.gpu
BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
ROWS = [1, 31, 32, 33, 127, 128, 129, 257, 389]
PFN_ROWS = [1, 127, 128, 129, 389]
KN = [(k, n) for k in (32, 64, 128) for n in (32, 64, 128)]
CUS = 256


def _dev():
    return torch.device('cuda:0')


# ---- comparison, uploads --------------------------------------------------------------------------------------------------------------------
def _same(got, want_i64, dtype, what, explain=None):
    """got (GPU tensor) == the int64 reference cast to `dtype`, at every element; shape and dtype asserted too."""
    want = R.rounded_bf16(want_i64) if dtype == BF16 else R.exact_f32(want_i64)
    assert got.dtype == dtype, '%s: dtype %s, expected %s' % (what, got.dtype, dtype)
    assert tuple(got.shape) == tuple(want.shape), '%s: shape %s, expected %s' % (what, tuple(got.shape), tuple(want.shape))
    g = got.detach().cpu().contiguous()
    if torch.equal(g, want):
        return
    bad = ~(g == want)                                         # a NaN is bad too
    first = tuple(int(v) for v in bad.nonzero()[0])
    msg = '%s: %d of %d elements differ; first at %s: kernel %r, exact %r' % (what, int(bad.sum()), bad.numel(), first, float(g[first]), float(want[first]))
    if explain is not None:
        msg += '\n  ' + explain(first, float(g[first]))
    raise AssertionError(msg)


def _up(t, dtype):
    """An operand to the GPU in `dtype`: int64 through the exact casts, float tensors (masks, ReLU edges) as they are."""
    if t is None:
        return None
    if t.dtype == I64:
        return (R.exact_bf16(t) if dtype == BF16 else R.exact_f32(t)).to(_dev())
    out = t.to(dtype)
    assert torch.equal(out.float().nan_to_num(7.0), t.float().nan_to_num(7.0)), 'a float operand does not fit %s' % dtype
    return out.to(_dev())


def _f(t):
    return _up(t, F32)


def _i32(t):
    return None if t is None else t.to(torch.int32).to(_dev())


def _amax(t):
    return native.absmax256(t) if t.numel() else torch.zeros((256,), dtype=F32, device=t.device)


def _amax_is(y_amax, y_i64, what):
    assert float(y_amax.max()) == float(y_i64.abs().max()), '%s: max of the 256 partial maxima %r, max |y| %r' % (what, float(y_amax.max()), float(y_i64.abs().max()))


@pytest.fixture
def switches(monkeypatch):
    """set(**env): launcher switches through the environment, re-read at once; undone (and re-read) afterwards."""
    def set_(**env):
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        native.reload_switches()
    yield set_
    monkeypatch.undo()
    native.reload_switches()


def _seed(*v):
    return sum((i + 1) * int(x) for i, x in enumerate(v)) % 9973 + 1


def _pooled_rows(rows):
    return 2 * (rows // 6 + 1)                                  # an even number of pooled rows, fewer than points from 4 rows on


def _explainer(f, wide):
    return lambda where, got: R.explain_position(f, where, got, wide)


# =========================================================================================================================================
# CPU self-checks
# =========================================================================================================================================
@pytest.mark.parametrize('rows,k,n', [(5, 8, 6), (1, 4, 4), (37, 16, 9)])
def test_reference_matches_the_library_in_float64(rows, k, n):
    """linear and wgrad_aug == F.linear and its float64 autograd on the same integers: masks, pre- and post-ReLU, residual, the cat forms."""
    f = R.dense_small(3, rows, k, n, wmax=2)
    x, w, b, res = f['x'], f['w'], f['bias'], f['residual']
    gy = R.small_grad(6, (rows, n))
    xd, wd, bd, rd = (t.double().requires_grad_(True) for t in (x, w, b, res))
    y = torch.relu(torch.nn.functional.linear(torch.relu(xd), wd, bd) + rd)
    y.backward(gy.double())
    y_int = R.linear(x, w, b, res, pre_relu=True, post_relu=True)
    assert torch.equal(y_int.double(), y.detach())
    assert torch.equal(R.linear(gy, w.t().contiguous(), in_mask=y_int, out_mask=x).double(), xd.grad)          # the backward-data form
    aug = R.wgrad_aug(gy, x, dy_mask=y_int, x_relu=True)
    dw, db = R.split_layout(aug)
    assert torch.equal(dw.double(), wd.grad) and torch.equal(db.double(), bd.grad)
    im, om = R.relu_like_mask(4, x.shape), R.relu_like_mask(5, (rows, n))
    assert torch.equal(R.linear(x, w, in_mask=im, out_mask=om).double(), torch.nn.functional.linear((x * (im > 0)).double(), w.double()) * (om > 0))
    # two-piece rows, forward and the split backward
    m, ka = 4, k // 2
    xa, xb, idx = x[:, :ka].contiguous(), R.small_grad(8, (m, k - ka)), R.gather_index(2, rows, m)
    xc = R.cat_rows(xa, xb, idx)
    own = R.small_grad(9, (rows, k - ka))
    assert torch.equal(xc, torch.cat([xa, xb[idx.long()]], 1)) and torch.equal(R.cat_rows(xa, own), torch.cat([xa, own], 1)) and R.cat_rows(xa) is xa
    xcd = xc.double().requires_grad_(True)
    torch.nn.functional.linear(torch.relu(xcd), w.double()).backward(gy.double())
    ya, yb = R.linear_cat_backward(gy, w.t().contiguous(), ka, None, xa, xb, idx)
    assert torch.equal(torch.cat([ya, yb], 1).double(), xcd.grad)


def test_pfn_reference_matches_resnet_block_in_float64():
    """pfn_forward / pfn_backward == ResnetBlockFC(64, 32) (pcaccumulation_amd/pillar_encoder.py, its unfused branch on the CPU) and autograd in float64."""
    from pcaccumulation_amd.pillar_encoder import ResnetBlockFC
    rows = 23
    x, _, _ = R.pfn_inputs(5, rows)
    w0, b0, ws, w1, b1 = R.pfn_weights(7)
    blk = ResnetBlockFC(64, 32).double()
    with torch.no_grad():
        for p, v in ((blk.fc_0.weight, w0), (blk.fc_0.bias, b0), (blk.shortcut.weight, ws), (blk.fc_1.weight, w1), (blk.fc_1.bias, b1)):
            p.copy_(v.double())
    xd = x.double().requires_grad_(True)
    out = blk(xd)
    gout = R.small_grad(9, (rows, 32))
    out.backward(gout.double())
    fwd = R.pfn_forward(x, w0, b0, ws, w1, b1)
    assert torch.equal(fwd['out'].double(), out.detach())
    assert torch.equal(fwd['relu_h'].double(), torch.relu(torch.nn.functional.linear(torch.relu(x.double()), w0.double(), b0.double())))
    for r in range(rows):
        assert [c for c in range(64) if (int(fwd['xmask'][r]) >> c) & 1] == (x[r] > 0).nonzero().view(-1).tolist()
        assert [c for c in range(32) if (int(fwd['hmask'][r]) >> c) & 1] == (fwd['relu_h'][r] > 0).nonzero().view(-1).tolist()
    bwd = R.pfn_backward(x, fwd['relu_h'], gout, w0, ws, w1)
    assert torch.equal(bwd['grad_x'].double(), xd.grad)
    want = torch.cat([blk.fc_1.weight.grad.view(-1), blk.fc_1.bias.grad, blk.shortcut.weight.grad.view(-1), blk.fc_0.weight.grad.view(-1), blk.fc_0.bias.grad])
    assert bwd['params'].numel() == 5184 and torch.equal(bwd['params'].double(), want)
    assert [name for name, _ in R.PFN_ORDER] == [k for k, _ in sorted(native.PFN_BLOCK_SLICES.items(), key=lambda kv: kv[1][0])]


def test_families_hold_their_own_conditions():
    """Every family passes its own assertions at the widest shapes it is used with; an input that is NOT exact is refused."""
    for k, n in ((32, 32), (128, 128)):
        R.dense_small(1, 389, k, n)
        R.lo_activations(2, 389, k, n)
        R.lo_activations(2, 129, k, n, one_large=True)
        R.lo_weights(3, 129, k, n)
        R.bf16_mantissa(4, 129, k, n)
        R.bf16_ties(5, 129, k, n)
        R.weight_rounding(6, 129, k, n)
        R.lo_pieces(7, 129, k // 2, k // 2, 44, n)
    one = R.lo_activations(2, 129, 64, 64, one_large=True)['x']
    assert R.lo_count(one) >= 1 and int((one.abs() > 511).sum()) == 1
    for rows in (4, 129):
        idx = R.gather_index(3, rows, _pooled_rows(rows))
        assert idx.dtype == torch.int32 and int(idx[0]) == _pooled_rows(rows) - 1 and int(idx[-1]) == 0
    m = R.mask_edges(1, (5, 32))
    assert {repr(float(v)) for v in m.view(-1)} == {repr(v) for v in R.MASK_EDGES}
    assert R.keep(torch.tensor(R.MASK_EDGES + (float('nan'),))).tolist() == [False, False, False, True, True, False]
    xf, xi = R.relu_edges(2, (4, 8))
    assert torch.equal(xf.to(I64), xi) and bool(torch.signbit(xf.view(-1)[1]))
    x, ws_ = R.pfn_wide_h(3, 129)
    with pytest.raises(R.NotExact):
        R.linear(torch.full((1, 32), 1 << 20, dtype=I64), torch.ones((32, 32), dtype=I64))
    with pytest.raises(AssertionError):
        R.assert_one_lo_per_product(torch.tensor([[(1 << 20) - 1]]), torch.tensor([[(1 << 19) + 1]]))
    assert R.round_bf16(torch.tensor([257, 259, 261, 258, -511])).tolist() == [256, 260, 260, 258, -512]
    # the double rounding of the bf16 residual path is visible to the reference: 257 -> 256, + 1 = 257 -> 256; rounded once, 258
    y = R.linear(torch.tensor([[1]]), torch.tensor([[257]]), None, torch.tensor([[1]]), bf16=True)
    assert y.tolist() == [[256]] and R.linear(torch.tensor([[1]]), torch.tensor([[257]]), None, torch.tensor([[1]])).tolist() == [[258]]


def test_position_code_names_the_element_that_was_read():
    f = R.position_code(1, 9, 16, 32, 16, 4, wide=True)
    x = R.cat_rows(f['xa'], f['xb'], f['b_index'])
    y = R.linear(x, f['w'])
    for row, o in ((0, 0), (8, 31), (4, 7)):
        c = int(f['src'][o])
        v = int(y[row, o])
        assert v == int(x[row, c])
        piece, prow, col = v >> 20, ((v - 1) >> 7) & 8191, (v - 1) & 127
        assert (piece, col) == ((0, c) if c < 16 else (1, c - 16)) and prow == (row if c < 16 else int(f['b_index'][row]))
    o = int((f['src'] >= 16).nonzero()[0])                       # an output that reads the pooled piece
    wrong = int(f['xb'][int(f['b_index'][3]) ^ 1, int(f['src'][o]) - 16])
    text = R.explain_position(f, (3, o), float(wrong), wide=True)
    assert 'reads piece 1 (row %d' % int(f['b_index'][3]) in text and 'the kernel gave %d = piece 1 (row %d' % (wrong, int(f['b_index'][3]) ^ 1) in text
    assert 'which no input element holds' in R.explain_position(f, (3, o), 0.5, wide=True)
    narrow = R.position_code(1, 9, 16, 32, 16, 4)
    assert int(narrow['xa'].min()) >= 1 and int(narrow['xa'].max()) <= 255 and R.exact_bf16(narrow['xb']) is not None


# =========================================================================================================================================
# forward, bf16 (mlp_mfma.hip) and fp32x3 (mlp_split.hip): one body, two modes
# =========================================================================================================================================
def _lin(mode, x, w, bias=None, residual=None, pre=False, post=False, in_mask=None, out_mask=None, x_float=None):
    """The plain forward entry point of `mode` ('bf16' | 'x3') on int64 operands (x_float: the float form of x, for -0.0) -> GPU result."""
    dt = BF16 if mode == 'bf16' else F32
    xg = _up(x_float if x_float is not None else x, dt)
    if mode == 'bf16':
        return native.rows_linear(xg, _f(w), _f(bias), _up(residual, dt), pre, post, _up(in_mask, dt), _up(out_mask, dt))
    return native.rows_linear_split(xg, _amax(xg), _f(w), _f(bias), _up(residual, dt), pre, post, _up(in_mask, dt), _up(out_mask, dt))


def _forward_case(mode, k, n, rows, nan=False):
    bf = mode == 'bf16'
    dt = BF16 if bf else F32
    wide = not bf
    sd = _seed(k, n, rows)
    wq = R.bf16_weights if bf else (lambda w: w)
    tag = '%s %dx%d rows %d ' % (mode, k, n, rows)
    # 1 dense: everything on, everything off
    f = R.dense_small(sd, rows, k, n)
    x, w, b, res = f['x'], f['w'], f['bias'], f['residual']
    _same(_lin(mode, x, w, b, res, True, True), R.linear(x, w, b, res, True, True, bf16=bf), dt, tag + 'dense bias residual relus')
    _same(_lin(mode, x, w), R.linear(x, w, bf16=bf), dt, tag + 'dense plain')
    # 7 mask edges on both masks; ReLU edges on x
    im, om = R.mask_edges(sd + 1, (rows, k), nan), R.mask_edges(sd + 2, (rows, n), nan)
    _same(_lin(mode, x, w, b, None, False, False, im, om), R.linear(x, w, b, None, False, False, im, om, bf16=bf), dt, tag + 'mask edges')
    xf, xi = R.relu_edges(sd + 3, (rows, k))
    _same(_lin(mode, xi, w, b, None, True, True, x_float=xf), R.linear(xi, w, b, None, True, True, bf16=bf), dt, tag + 'relu edges')
    # 2 position code
    p = R.position_code(sd, rows, k, n, wide=wide)
    _same(_lin(mode, p['xa'], p['w']), R.linear(p['xa'], p['w'], bf16=bf), dt, tag + 'position', _explainer(p, wide))
    # 4 mantissa, 6 weight rounding
    f = R.bf16_mantissa(sd, rows, k, n)
    _same(_lin(mode, f['x'], f['w'], f['bias']), R.linear(f['x'], f['w'], f['bias'], bf16=bf), dt, tag + 'mantissa')
    f = R.weight_rounding(sd, rows, k, n)
    _same(_lin(mode, f['x'], f['w']), R.linear(f['x'], wq(f['w']), bf16=bf), dt, tag + 'weight rounding')
    if bf:
        f = R.bf16_ties(sd, rows, k, n)                                                          # 5
        _same(_lin(mode, f['x'], f['w'], f['bias']), R.linear(f['x'], f['w'], f['bias'], bf16=True), dt, tag + 'ties')
        f = R.bf16_mantissa(sd + 5, rows, k, n)                                                  # the residual path rounds twice
        res = R.small_grad(sd + 6, (rows, n), -128, 127)
        _same(_lin(mode, f['x'], f['w'], f['bias'], res, False, True), R.linear(f['x'], f['w'], f['bias'], res, False, True, bf16=True), dt, tag + 'residual')
    else:
        for name, f in (('lo x', R.lo_activations(sd, rows, k, n)), ('lo x, one large', R.lo_activations(sd, rows, k, n, one_large=True)),
                        ('lo w', R.lo_weights(sd, rows, k, n))):                                 # 3
            _same(_lin(mode, f['x'], f['w']), R.linear(f['x'], f['w']), dt, tag + name)
        # second outputs: y_amax, and y16 = RNE(y) bit for bit ('mixed' mode)
        f = R.bf16_mantissa(sd, rows, k, n)
        xg = _f(f['x'])
        want = R.linear(f['x'], f['w'], f['bias'], None, False, True)
        y, y_amax = native.rows_linear_split(xg, _amax(xg), _f(f['w']), _f(f['bias']), None, False, True, want_amax=True)
        _same(y, want, F32, tag + 'y with y_amax')
        _amax_is(y_amax, want, tag + 'y_amax')
        y, y_amax, y16 = native.rows_linear_split(xg, _amax(xg), _f(f['w']), _f(f['bias']), None, False, True, want_bf16=True)
        _same(y, want, F32, tag + 'dual y')
        _same(y16, want, BF16, tag + 'dual y16')
        _amax_is(y_amax, want, tag + 'dual y_amax')


def _cat_case(mode, k, n, rows, nan=False):
    bf = mode == 'bf16'
    dt = BF16 if bf else F32
    wide = not bf
    sd = _seed(k, n, rows, 7)
    ka = k // 2 if sd % 2 else 8
    kb, m = k - ka, _pooled_rows(rows)
    tag = '%s cat %d+%d->%d rows %d ' % (mode, ka, kb, n, rows)

    def fwd(xa, xb, idx, w, bias=None, residual=None, pre=False, post=False):
        a, b_ = _up(xa, dt), _up(xb, dt)
        if bf:
            return native.rows_linear_cat(a, b_, _i32(idx), _f(w), _f(bias), _up(residual, dt), pre, post)
        return native.rows_linear_cat_split(a, _amax(a), b_, _amax(b_), _i32(idx), _f(w), _f(bias), _up(residual, dt), pre, post)

    p = R.position_code(sd, rows, ka, n, kb, m, wide=wide)
    _same(fwd(p['xa'], p['xb'], p['b_index'], p['w']), R.linear(R.cat_rows(p['xa'], p['xb'], p['b_index']), p['w'], bf16=bf), dt, tag + 'position',
          _explainer(p, wide))
    q = dict(p, xb=R.position_value(1, torch.arange(rows).view(-1, 1), torch.arange(kb).view(1, -1), wide), b_index=None)       # b_index = None: xb[row]
    _same(fwd(q['xa'], q['xb'], None, q['w']), R.linear(R.cat_rows(q['xa'], q['xb']), q['w'], bf16=bf), dt, tag + 'position, no index', _explainer(q, wide))
    f = R.dense_small(sd, rows, k, n)
    xa, xb, idx = f['x'][:, :ka].contiguous(), R.small_grad(sd + 1, (m, kb)), R.gather_index(sd, rows, m)
    _same(fwd(xa, xb, idx, f['w'], f['bias'], f['residual'], True, True),
          R.linear(R.cat_rows(xa, xb, idx), f['w'], f['bias'], f['residual'], True, True, bf16=bf), dt, tag + 'dense bias residual relus')
    if not bf:
        f = R.lo_pieces(sd, rows, ka, kb, m, n)
        a, b_ = _f(f['xa']), _f(f['xb'])
        want = R.linear(R.cat_rows(f['xa'], f['xb'], f['b_index']), f['w'])
        y, y_amax = native.rows_linear_cat_split(a, _amax(a), b_, _amax(b_), _i32(f['b_index']), _f(f['w']), want_amax=True)
        _same(y, want, F32, tag + 'pooled piece 2^10 above the point piece')
        _amax_is(y_amax, want, tag + 'y_amax')
    # the backward-data form: kernel (k, n) = gy [rows, k] -> [rows, n] split at na into y / y2, masked by cat(out_mask_a, out_mask_b[b_index])
    na = n // 2 if sd % 2 else n - 8
    nb = n - na
    p = R.position_code(sd + 2, rows, k, n, wide=wide)                                            # result column o reads gy column src[o]
    oma, omb = R.mask_edges(sd + 3, (rows, na), nan), R.mask_edges(sd + 4, (m, nb), nan)
    dym = R.mask_edges(sd + 5, (rows, k), nan)
    for name, gy, wt in (('position', p['xa'], p['w']), ('dense', R.small_grad(sd + 6, (rows, k)), R.small_grad(sd + 7, (n, k), -1, 1))):
        g = _up(gy, dt)
        args = (_f(wt), _up(dym, dt), _up(oma, dt), _up(omb, dt), _i32(idx), True)
        if bf:
            ya, yb = native.rows_linear_cat_backward(g, *args)
        else:
            ya, yb, g_amax = native.rows_linear_cat_backward_split(g, _amax(g), *args)
        wa, wb = R.linear_cat_backward(gy, wt, na, dym, oma, omb, idx, bf16=bf)
        _same(ya, wa, dt, tag + 'backward %s y (na %d)' % (name, na))
        _same(yb, wb, dt, tag + 'backward %s y2' % name)
        if not bf:
            _amax_is(g_amax, torch.cat([wa, wb], 1), tag + 'backward y_amax')


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('k,n', KN)
def test_bf16_forward(k, n, rows):
    _forward_case('bf16', k, n, rows)
    _cat_case('bf16', k, n, rows)


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('k,n', KN)
def test_fp32x3_forward(k, n, rows):
    _forward_case('x3', k, n, rows)
    _cat_case('x3', k, n, rows)


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('k,n', [(128, 128), (128, 64), (64, 128)])
def test_fp32x3_forward_weights_in_lds(k, n, rows, switches):
    """The three wide shapes on rows_linear_split_kernel (PCACC_ROWS_FM_OFF) instead of the weights-in-registers kernel."""
    switches(PCACC_ROWS_FM_OFF='1')
    _forward_case('x3', k, n, rows)
    _cat_case('x3', k, n, rows)


def _bf16_per_cu(k, n):
    lds = (128 * (max(k, n) + 8) + n * (k + 8)) * 2 + n * 4
    return max(1, min(4, (160 * 1024) // lds))


def _x3_per_cu(k, n):
    region = max(2 * 128 * (k + 8) * 2, 128 * (n + 4) * 4)
    return max(1, min(3, (160 * 1024) // (region + 2 * n * (k + 8) * 2 + 3 * n * 4)))


def _persistent_case(mode, k, n, rows):
    """More tiles than the grid: position code (which tile did a row come from?) and dense with residual and out_mask."""
    bf = mode == 'bf16'
    dt = BF16 if bf else F32
    sd = _seed(k, n, rows)
    tag = '%s %dx%d persistent rows %d ' % (mode, k, n, rows)
    p = R.position_code(sd, rows, k, n, wide=not bf)
    _same(_lin(mode, p['xa'], p['w']), R.linear(p['xa'], p['w'], bf16=bf), dt, tag + 'position', _explainer(p, not bf))
    f = R.dense_small(sd, rows, k, n)
    om = R.relu_like_mask(sd + 1, (rows, n))
    _same(_lin(mode, f['x'], f['w'], f['bias'], f['residual'], True, False, None, om),
          R.linear(f['x'], f['w'], f['bias'], f['residual'], True, False, None, om, bf16=bf), dt, tag + 'dense')
    ka, m = k // 2, 1000
    q = R.position_code(sd, rows, ka, n, k - ka, m, wide=not bf)
    a, b_ = _up(q['xa'], dt), _up(q['xb'], dt)
    y = (native.rows_linear_cat(a, b_, _i32(q['b_index']), _f(q['w'])) if bf
         else native.rows_linear_cat_split(a, _amax(a), b_, _amax(b_), _i32(q['b_index']), _f(q['w'])))
    _same(y, R.linear(R.cat_rows(q['xa'], q['xb'], q['b_index']), q['w'], bf16=bf), dt, tag + 'cat position', _explainer(q, not bf))


@gpu
@pytest.mark.parametrize('k,n', KN)
def test_bf16_forward_persistent(k, n):
    _persistent_case('bf16', k, n, 128 * CUS * _bf16_per_cu(k, n) + 129)


@gpu
@pytest.mark.parametrize('k,n', KN)
def test_fp32x3_forward_persistent(k, n):
    fm = (k, n) in ((128, 128), (128, 64), (64, 128))
    _persistent_case('x3', k, n, 128 * CUS * (2 if fm else _x3_per_cu(k, n)) + 129)


@gpu
@pytest.mark.parametrize('k,n', [(128, 128), (128, 64), (64, 128)])
def test_fp32x3_forward_persistent_weights_in_lds(k, n, switches):
    switches(PCACC_ROWS_FM_OFF='1')
    _persistent_case('x3', k, n, 128 * CUS * _x3_per_cu(k, n) + 129)


def test_grid_caps_follow_the_launchers():
    """per_cu of mm_launch / ms_launch as the docstring states it (the persistent cases rely on it)."""
    assert [_bf16_per_cu(k, n) for k, n in KN] == [4, 4, 3, 4, 4, 3, 3, 3, 2]
    assert [_x3_per_cu(k, n) for k, n in KN] == [3, 3, 1, 3, 2, 1, 1, 1, 1]
    assert (_bf16_per_cu(128, 64), _x3_per_cu(64, 64)) == ((160 * 1024) // 52480, (160 * 1024) // 56064)      # two of them by hand, from the LDS bytes


# =========================================================================================================================================
# weight gradients, bf16 and fp32x3
# =========================================================================================================================================
def _wg(mode, dy, x, dy_mask=None, x_relu=False, split=False, cat=None):
    dt = BF16 if mode == 'bf16' else F32
    g, m = _up(dy, dt), _up(dy_mask, dt)
    if cat is None:
        xg = _up(x, dt)
        if mode == 'bf16':
            return native.rows_wgrad(g, xg, m, x_relu, split)
        return native.rows_wgrad_split(g, _amax(g), xg, _amax(xg), m, x_relu, split)
    xa, xb, idx = cat
    a, b_ = _up(xa, dt), _up(xb, dt)
    if mode == 'bf16':
        return native.rows_wgrad_cat(g, a, b_, _i32(idx), m, x_relu, split)
    return native.rows_wgrad_cat_split(g, _amax(g), a, _amax(a), b_, _amax(b_), _i32(idx), m, x_relu, split)


def _same_wgrad(got, aug, split, what, layout=True):
    """layout: the kernel itself wrote dW followed by db (the matrix-core kernels and rows_wgrad_few on at least one row)."""
    if split:
        dw, db = R.split_layout(aug)
        _same(got[0], dw, F32, what + ' dW')
        _same(got[1], db, F32, what + ' db')
        if layout:
            assert got[0].is_contiguous() and got[1].is_contiguous() and got[1].data_ptr() == got[0].data_ptr() + 4 * dw.numel(), what + ': not dW followed by db'
    else:
        _same(got, aug, F32, what)


def _sparse_rows(seed, rows, cols, per_col=6):
    """20-bit odd values at `per_col` rows of every column (zero elsewhere): a lo-plane operand of a reduction over rows."""
    g = R._gen(seed)
    t = torch.zeros((rows, cols), dtype=I64)
    idx = torch.randint(0, rows, (min(rows, per_col), cols), generator=g)
    mag = R._randint(g, 1 << 17, (1 << 20) - 1, idx.shape) | 1
    t.scatter_(0, idx, mag * (R._randint(g, 0, 1, idx.shape) * 2 - 1))
    return t


def _wgrad_case(mode, k, n, rows, nan=False):
    sd = _seed(k, n, rows, 11)
    tag = '%s wgrad %dx%d rows %d ' % (mode, k, n, rows)
    dy, x = R.small_grad(sd, (rows, n)), R.small_grad(sd + 1, (rows, k))
    edge, relu_m = R.mask_edges(sd + 2, (rows, n), nan), R.relu_like_mask(sd + 3, (rows, n))
    _same_wgrad(_wg(mode, dy, x), R.wgrad_aug(dy, x), False, tag + 'dense')
    _same_wgrad(_wg(mode, dy, x, edge, True, True), R.wgrad_aug(dy, x, edge, True), True, tag + 'mask edges, x_relu, split layout')
    _same_wgrad(_wg(mode, dy, x, relu_m, False, False), R.wgrad_aug(dy, x, relu_m), False, tag + 'relu-like mask')
    xf, xi = R.relu_edges(sd + 4, (rows, k))
    dt = BF16 if mode == 'bf16' else F32
    g, xg = _up(dy, dt), _up(xf, dt)
    got = native.rows_wgrad(g, xg, None, True, False) if mode == 'bf16' else native.rows_wgrad_split(g, _amax(g), xg, _amax(xg), None, True, False)
    _same_wgrad(got, R.wgrad_aug(dy, xi, None, True), False, tag + 'relu edges')
    # position: dy one-hot per row -> dW[o] sums the rows that chose o; 8-bit / 20-bit operands
    f = R.bf16_mantissa(sd, rows, k, n)
    _same_wgrad(_wg(mode, R.small_grad(sd + 5, (rows, n), -1, 1), f['x'], None, False, True), R.wgrad_aug(R.small_grad(sd + 5, (rows, n), -1, 1), f['x']), True,
                tag + 'mantissa x')
    if mode == 'x3':
        lo_g, lo_x = _sparse_rows(sd + 6, rows, n), _sparse_rows(sd + 7, rows, k)
        ones_x, ones_g = R.small_grad(sd + 8, (rows, k), -1, 1), R.small_grad(sd + 9, (rows, n), -1, 1)
        assert R.lo_count(lo_g) > 0 and R.lo_count(lo_x) > 0
        _same_wgrad(_wg(mode, lo_g, ones_x), R.wgrad_aug(lo_g, ones_x), False, tag + 'lo dy')
        _same_wgrad(_wg(mode, ones_g, lo_x, relu_m), R.wgrad_aug(ones_g, lo_x, relu_m), False, tag + 'lo x')
    # two-piece x
    ka, m = (k // 2 if sd % 2 else 8), _pooled_rows(rows)
    xa, xb, idx = x[:, :ka].contiguous(), R.small_grad(sd + 10, (m, k - ka)), R.gather_index(sd, rows, m)
    xc = R.cat_rows(xa, xb, idx)
    _same_wgrad(_wg(mode, dy, None, edge, True, True, (xa, xb, idx)), R.wgrad_aug(dy, xc, edge, True), True, tag + 'cat, split layout')
    _same_wgrad(_wg(mode, dy, None, None, False, False, (xa, R.small_grad(sd + 10, (rows, k - ka)), None)),
                R.wgrad_aug(dy, R.cat_rows(xa, R.small_grad(sd + 10, (rows, k - ka)))), False, tag + 'cat, no index')
    if mode == 'x3':
        f = R.lo_pieces(sd, rows, ka, k - ka, m, n)
        g1 = R.small_grad(sd + 11, (rows, n), -1, 1) * (R.small_grad(sd + 12, (rows, n), 0, 40) == 0)        # sparse in rows: sum |term| stays below 2^24
        _same_wgrad(_wg(mode, g1, None, None, False, False, (f['xa'], f['xb'], f['b_index'])), R.wgrad_aug(g1, R.cat_rows(f['xa'], f['xb'], f['b_index'])), False,
                    tag + 'cat, pooled piece 2^10 above')


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('k,n', KN)
def test_bf16_wgrad(k, n, rows):
    _wgrad_case('bf16', k, n, rows)


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('k,n', KN)
def test_fp32x3_wgrad(k, n, rows):
    _wgrad_case('x3', k, n, rows)


@gpu
@pytest.mark.parametrize('mode,k,n,tile', [('bf16', 32, 32, 256), ('bf16', 64, 64, 128), ('bf16', 128, 128, 64), ('x3', 64, 64, 128), ('x3', 128, 128, 64),
                                           ('x3', 32, 128, 64)])
def test_wgrad_more_chunks_than_the_grid(mode, k, n, tile):
    """One case per tile height with more chunks than workgroups (grid cap 1024 / at most 768): the partial slots and the reduce over all of them."""
    rows = 1024 * tile + tile + 5
    sd = _seed(k, n, tile)
    dy, x, mk = R.small_grad(sd, (rows, n), -2, 2), R.small_grad(sd + 1, (rows, k), -2, 2), R.relu_like_mask(sd + 2, (rows, n))
    _same_wgrad(_wg(mode, dy, x, mk, True, True), R.wgrad_aug(dy, x, mk, True), True, '%s wgrad %dx%d rows %d' % (mode, k, n, rows))
    m = 1000
    xa, xb, idx = x[:, :k // 2].contiguous(), R.small_grad(sd + 3, (m, k - k // 2), -2, 2), R.gather_index(sd, rows, m)
    _same_wgrad(_wg(mode, dy, None, None, False, False, (xa, xb, idx)), R.wgrad_aug(dy, R.cat_rows(xa, xb, idx)), False, '%s wgrad cat %dx%d rows %d' % (mode, k, n, rows))


@gpu
@pytest.mark.parametrize('k,n', KN)
def test_wgrad_of_no_rows_is_zero(k, n):
    for mode in ('bf16', 'x3'):
        for split in (False, True):
            got = _wg(mode, torch.zeros((0, n), dtype=I64), torch.zeros((0, k), dtype=I64), None, False, split)
            _same_wgrad(got, torch.zeros((n, k + 1), dtype=I64), split, '%s wgrad %dx%d no rows' % (mode, k, n), layout=False)
    for kk, nn in ((9, 64), (64, 2), (16, 128)):
        got = native.rows_wgrad(torch.zeros((0, nn), device=_dev()), torch.zeros((0, kk), device=_dev()))
        _same(got, torch.zeros((nn, kk + 1), dtype=I64), F32, 'fp32 wgrad %dx%d no rows' % (kk, nn))


# =========================================================================================================================================
# fp32 kernels (mlp.hip)
# =========================================================================================================================================
def _fp32_forward(k, n, rows, dts=(F32,) * 5, nan=False, few_big=False):
    """rows_linear through the fp32-arithmetic kernels with element types (x, in_mask, residual, out_mask, y); bf16 tensors get 8-bit values."""
    dx, dim, dres, dom, dy_ = dts
    sd = _seed(k, n, rows, 13)
    tag = 'fp32 %dx%d rows %d %s ' % (k, n, rows, ''.join('b' if d == BF16 else 'f' for d in dts))
    wide = dx == F32
    f = R.dense_small(sd, rows, k, n, wmax=2)
    x, w, b, res = f['x'], f['w'], f['bias'], f['residual']
    im, om = R.mask_edges(sd + 1, (rows, k), nan), R.mask_edges(sd + 2, (rows, n), nan)

    def run(x, w, b=None, res=None, pre=False, post=False, im=None, om=None, xf=None):
        return native.rows_linear(_up(xf if xf is not None else x, dx), _f(w), _f(b), _up(res, dres), pre, post, _up(im, dim), _up(om, dom), out_dtype=dy_)

    _same(run(x, w, b, res, True, True), R.linear(x, w, b, res, True, True), dy_, tag + 'dense bias residual relus')
    _same(run(x, w, b, None, False, False, im, om), R.linear(x, w, b, None, False, False, im, om), dy_, tag + 'mask edges')
    xf, xi = R.relu_edges(sd + 3, (rows, k))
    _same(run(xi, w, b, None, True, True, xf=xf), R.linear(xi, w, b, None, True, True), dy_, tag + 'relu edges')
    p = R.position_code(sd, rows, k, n, wide=wide)
    if dy_ == F32 or not wide:
        _same(run(p['xa'], p['w']), R.linear(p['xa'], p['w']), dy_, tag + 'position', _explainer(p, wide))
    f = R.weight_rounding(sd, rows, k, n) if k >= 4 else None
    if f is not None:
        _same(run(f['x'], f['w']), R.linear(f['x'], f['w']), dy_, tag + 'weights stay fp32')                 # fp32 arithmetic: 257 stays 257
    if dy_ == BF16:
        f = R.bf16_ties(sd, rows, k, n) if k >= 4 else None
        if f is not None:
            _same(run(f['x'], f['w'], f['bias']), R.linear(f['x'], f['w'], f['bias']), BF16, tag + 'ties')   # one rounding, at the store


@gpu
@pytest.mark.parametrize('n', [3, 7, 33, 100, 128])
@pytest.mark.parametrize('k', [2, 3, 4, 9, 32, 64, 128])
def test_fp32_forward_generic(k, n):
    """rows_linear_kernel<K, 128> (max(k, n) <= 64) / <K, 64>; k <= 9 with n = 128 is the few-input kernel, covered below too."""
    tile = 128 if max(k, n) <= 64 else 64
    for rows in (1, tile - 1, tile, tile + 1, 2 * tile + 1, 389):
        _fp32_forward(k, n, rows)


@gpu
@pytest.mark.parametrize('k,n,tile', [(32, 33, 128), (9, 100, 64)])
def test_fp32_forward_generic_persistent(k, n, tile):
    rows = 16 * CUS * tile + tile + 1
    sd = _seed(k, n, tile)
    p = R.position_code(sd, rows, k, n, wide=True)
    _same(native.rows_linear(_f(p['xa']), _f(p['w'])), R.linear(p['xa'], p['w']), F32, 'fp32 %dx%d persistent position' % (k, n), _explainer(p, True))
    f = R.dense_small(sd, rows, k, n)
    _same(native.rows_linear(_f(f['x']), _f(f['w']), _f(f['bias']), _f(f['residual']), True, True), R.linear(f['x'], f['w'], f['bias'], f['residual'], True, True),
          F32, 'fp32 %dx%d persistent dense' % (k, n))


@gpu
@pytest.mark.parametrize('n', [8, 16, 32, 64, 128])
@pytest.mark.parametrize('k', [2, 3, 4, 9])
def test_fp32_forward_few_inputs(k, n):
    """rows_linear_fewk_kernel<K, n / 8, HALVES>: fp32 y (HALVES), bf16 y, and rows_linear_few_dual's y16 / y_amax."""
    big = 8 * CUS * 256 * 4 // (n // 8) + 3                       # more work items than the grid (2048 workgroups x 256 lanes x FEW_U = 4 rows) holds
    for rows in (1, 63, 64, 65, 389) + ((big,) if k == 9 else ()):
        _fp32_forward(k, n, rows)
        if rows != big:
            _fp32_forward(k, n, rows, (F32, F32, F32, F32, BF16))
            _fp32_forward(k, n, rows, (BF16, BF16, BF16, BF16, BF16))
        sd = _seed(k, n, rows, 17)
        x = R.small_grad(sd, (rows, k), -255, 255)
        w, b, res = R.small_grad(sd + 1, (n, k), -2, 2), R.small_grad(sd + 2, (n,), -4, 4), R.small_grad(sd + 3, (rows, n), -4, 4)
        want = R.linear(x, w, b, res, False, True)
        y, y_amax, y16 = native.rows_linear_few_dual(_f(x), _f(w), _f(b), _f(res), False, True)
        _same(y, want, F32, 'few_dual %dx%d rows %d y' % (k, n, rows))
        _same(y16, want, BF16, 'few_dual %dx%d rows %d y16' % (k, n, rows))
        _amax_is(y_amax, want, 'few_dual y_amax')
        assert R.bf16_rounding_census(want)[1] > 0 or rows < 8, 'few_dual: no inexact bf16 value in the result'


@gpu
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('k', [32, 64, 128])
def test_fp32_forward_few_outputs(k, n):
    for rows in (1, 31, 32, 33, 389, 16 * CUS * 256 // (k // 8) + 7):
        _fp32_forward(k, n, rows)
        _fp32_forward(k, n, rows, (BF16, BF16, F32, BF16, F32))


@gpu
@pytest.mark.parametrize('bits', [0, 1, 2, 4, 8, 16, 31])
def test_fp32_forward_element_types(bits):
    """The `dtypes` word of pcacc_rows_linear_mixed: all clear, each bit alone, all set (n = 33 keeps the all-bf16 call off the matrix-core kernel)."""
    dts = tuple(BF16 if bits & b else F32 for b in (1, 2, 4, 8, 16))
    for k, n, rows in ((32, 33, 129), (128, 100, 65), (9, 64, 257), (64, 2, 129)):
        _fp32_forward(k, n, rows, dts)


def _fp32_wgrad(k, n, rows, dts=(F32, F32, F32), nan=False):
    ddy, dm, dx = dts
    sd = _seed(k, n, rows, 19)
    tag = 'fp32 wgrad %dx%d rows %d %s ' % (k, n, rows, ''.join('b' if d == BF16 else 'f' for d in dts))
    dy, x = R.small_grad(sd, (rows, n)), R.small_grad(sd + 1, (rows, k))
    edge = R.mask_edges(sd + 2, (rows, n), nan)
    run = lambda dy, x, m=None, relu=False, split=False: native.rows_wgrad(_up(dy, ddy), _up(x, dx), _up(m, dm), relu, split)
    _same_wgrad(run(dy, x), R.wgrad_aug(dy, x), False, tag + 'dense')
    got = run(dy, x, edge, True, True)
    dw, db = R.split_layout(R.wgrad_aug(dy, x, edge, True))
    _same(got[0], dw, F32, tag + 'mask edges, x_relu dW')
    _same(got[1], db, F32, tag + 'mask edges, x_relu db')
    xf, xi = R.relu_edges(sd + 4, (rows, k))
    _same_wgrad(native.rows_wgrad(_up(dy, ddy), _up(xf, dx), None, True), R.wgrad_aug(dy, xi, None, True), False, tag + 'relu edges')
    top = 255 if rows <= 4096 else 15                            # rows * 255 would pass 2^24 on the long cases
    big_x = R.small_grad(sd + 5, (rows, k), -top, top)
    _same_wgrad(run(R.small_grad(sd + 6, (rows, n), -1, 1), big_x), R.wgrad_aug(R.small_grad(sd + 6, (rows, n), -1, 1), big_x), False, tag + 'mantissa x')


@gpu
@pytest.mark.parametrize('k,n,chunk,grid', [(32, 32, 96, 4 * CUS), (64, 48, 96, 2 * CUS), (16, 128, 32, 4 * CUS), (64, 64, 32, 2 * CUS), (128, 128, 32, 2 * CUS)])
def test_fp32_wgrad(k, n, chunk, grid):
    """rows_wgrad_kernel<96 | 32, T = 1 | 2 | 6> (fp32 MFMA, atomics into dw_aug), fp32 and mixed element types, more chunks than the grid."""
    for rows in (1, chunk - 1, chunk, chunk + 1, 389):
        _fp32_wgrad(k, n, rows)
    _fp32_wgrad(k, n, 129, (BF16, F32, F32))
    _fp32_wgrad(k, n, 129, (F32, BF16, F32))
    _fp32_wgrad(k, n, 129, (F32, F32, BF16))
    if n % 32 or k % 32:
        _fp32_wgrad(k, n, 129, (BF16, BF16, BF16))
    rows = grid * chunk + chunk + 1
    sd = _seed(k, n, chunk)
    dy, x, mk = R.small_grad(sd, (rows, n), -2, 2), R.small_grad(sd + 1, (rows, k), -2, 2), R.relu_like_mask(sd + 2, (rows, n))
    _same_wgrad(native.rows_wgrad(_f(dy), _f(x), _f(mk), True), R.wgrad_aug(dy, x, mk, True), False, 'fp32 wgrad %dx%d rows %d' % (k, n, rows))


@gpu
@pytest.mark.parametrize('c', [32, 64, 128])
@pytest.mark.parametrize('f', [1, 2, 3, 4, 9])
def test_fp32_wgrad_few(f, c):
    """rows_wgrad_few_kernel<F, C / 4, FAST>: few inputs (k = f) and few outputs (n = f); FAST 1 / 2 = bf16 dY (and bf16 mask) with fp32 X."""
    rb = 256 // (c // 4)
    big = 4 * CUS * 2 * rb + rb + 3                               # more tiles (FEW_WU = 2 x rb rows each) than the 1024 workgroups of wgrad_few_grid
    for rows in (1, rb - 1, rb, rb + 1, 389, big):
        _fp32_wgrad(f, c, rows)                                   # few inputs, FAST 0
        _fp32_wgrad(f, c, rows, (BF16, BF16, F32))                # FAST 1 (no mask) and 2 (mask)
        _fp32_wgrad(c, f, rows)                                   # few outputs
        if rows != big:
            _fp32_wgrad(f, c, rows, (BF16, F32, F32))             # bf16 dY, fp32 mask: FAST 0
            _fp32_wgrad(c, f, rows, (BF16, BF16, BF16))


# =========================================================================================================================================
# PFN block
# =========================================================================================================================================
def _pfn_x(xa, pooled, p2v):
    return xa if pooled is None else R.cat_rows(xa, pooled, p2v)


def _pfn_case(rows, gather, seed):
    m = _pooled_rows(rows) if gather else 0
    tag = 'pfn rows %d %s ' % (rows, 'gather' if gather else 'plain')
    long = rows > 4096                                          # the parameter gradients sum over all rows: +-1 operands keep them below 2^24
    top = 1 if long else 3
    xa, pooled, p2v = R.pfn_inputs(seed, rows, m, -top, top)
    wts = R.pfn_weights(seed + 1, 1 if long else 2)
    w0, b0, ws, w1, b1 = wts
    gout = R.small_grad(seed + 2, (rows, 32), -top, top)
    # --- bf16: out and relu_h are bf16 stores (h up to 388, d(x) up to 12000: both round); the backward holds d(h) as bf16
    bf_variants = [('dense', xa, pooled, wts)]
    if not long:
        ma, mp, _ = R.pfn_inputs(seed + 3, rows, m, -255, 255)      # all 8 bits of the mantissa; p2v = gather_index(seed + 3, ...) is not used, p2v above is
        bf_variants.append(('mantissa', ma, mp, R.pfn_weights(seed + 3, 1, sparse1=6)))
    for name, xa_, pooled_, wset in bf_variants:
        xx = _pfn_x(xa_, pooled_, p2v)
        q = [R.bf16_weights(t) for t in wset]
        fwd = R.pfn_forward(xx, *q, bf16=True)
        out, hr = native.pfn_block_forward(_up(xa_, BF16), _up(pooled_, BF16), _i32(p2v), *[_f(t) for t in wset])
        _same(out, fwd['out'], BF16, tag + 'bf16 %s out' % name)
        _same(hr, fwd['relu_h'], BF16, tag + 'bf16 %s relu_h' % name)
        g = gout if name == 'dense' else R.small_grad(seed + 4, (rows, 32), -1, 1)
        bwd = R.pfn_backward(xx, fwd['relu_h'], g, q[0], q[2], q[3], bf16=True)
        gxa, gxb, gp = native.pfn_block_backward(_up(xa_, BF16), _up(pooled_, BF16), _i32(p2v), hr, _up(g, BF16), _f(wset[0]), _f(wset[2]), _f(wset[3]))
        if gather:
            _same(gxa, bwd['grad_x'][:, :32].contiguous(), BF16, tag + 'bf16 %s grad_xa' % name)
            _same(gxb, bwd['grad_x'][:, 32:].contiguous(), BF16, tag + 'bf16 %s grad_xb' % name)
        else:
            _same(gxa, bwd['grad_x'], BF16, tag + 'bf16 %s grad_xa' % name)
            assert gxb is None
        _same(gp, bwd['params'], F32, tag + 'bf16 %s grad_params' % name)
    # --- fp32x3 and dual
    variants = [('dense', xa, pooled, wts)]
    lo_xa = R.small_grad(seed + 5, xa.shape, -(1 << 19), 1 << 19)
    lo_po = None if pooled is None else R.small_grad(seed + 6, pooled.shape, -(1 << 19), 1 << 19)
    g_ = R._gen(seed + 7)
    sparse = (R._sparse_signs(g_, (32, 64), 4), b0, R._sparse_signs(g_, (32, 64), 4), R._sparse_signs(g_, (32, 32), 2), b1)
    variants.append(('lo x', lo_xa, lo_po, sparse))
    if not gather and not long:
        xw, ww = R.pfn_wide_h(seed + 8, rows)
        variants.append(('h needs its lo half', xw, None, ww))
    for name, xa_, pooled_, wset in variants:
        xx = _pfn_x(xa_, pooled_, p2v)
        fwd = R.pfn_forward(xx, *wset)
        a, p_ = _f(xa_), _f(pooled_)
        gws = [_f(t) for t in wset]
        out, hr, xmask, hmask, out_amax, hr_amax = native.pfn_block_split_forward(a, _amax(a), p_, None if p_ is None else _amax(p_), _i32(p2v), *gws)
        _same(out, fwd['out'], F32, tag + 'x3 %s out' % name)
        _same(hr, fwd['relu_h'], F32, tag + 'x3 %s relu_h' % name)
        assert torch.equal(xmask.cpu(), fwd['xmask']), tag + 'x3 %s xmask' % name
        assert torch.equal(hmask.cpu().to(I64) & 0xffffffff, fwd['hmask']), tag + 'x3 %s hmask' % name
        _amax_is(out_amax, fwd['out'], tag + 'out_amax')
        _amax_is(hr_amax, fwd['relu_h'], tag + 'hr_amax')
        out2, out_amax2, out16, hr16 = native.pfn_block_split_forward_dual(a, _amax(a), p_, None if p_ is None else _amax(p_), _i32(p2v), *gws)
        _same(out2, fwd['out'], F32, tag + 'dual %s out' % name)
        _same(out16, fwd['out'], BF16, tag + 'dual %s out16' % name)
        _same(hr16, fwd['relu_h'], BF16, tag + 'dual %s hr16' % name)
        _amax_is(out_amax2, fwd['out'], tag + 'dual out_amax')
        if name == 'dense':
            bwd = R.pfn_backward(xx, fwd['relu_h'], gout, wset[0], wset[2], wset[3])
            gg = _f(gout)
            gxa, gxb, dh, gx_amax, dh_amax = native.pfn_block_split_dgrad(gg, _amax(gg), xmask, hmask, gws[0], gws[2], gws[3], gather)
            if gather:
                _same(gxa, bwd['grad_x'][:, :32].contiguous(), F32, tag + 'x3 grad_xa')
                _same(gxb, bwd['grad_x'][:, 32:].contiguous(), F32, tag + 'x3 grad_xb')
            else:
                _same(gxa, bwd['grad_x'], F32, tag + 'x3 grad_xa')
            _same(dh, bwd['grad_h'], F32, tag + 'x3 grad_h')
            _amax_is(gx_amax, bwd['grad_x'], tag + 'gx_amax')
            _amax_is(dh_amax, bwd['grad_h'], tag + 'dh_amax')


@gpu
@pytest.mark.parametrize('gather', [False, True])
@pytest.mark.parametrize('rows', PFN_ROWS + [768 * 128 + 129])
def test_pfn_block(rows, gather):
    _pfn_case(rows, gather, _seed(rows, gather, 23))


@gpu
@pytest.mark.parametrize('gather', [False, True])
def test_pfn_block_position(gather):
    """One-hot shortcut weights, w0 = w1 = 0: out[row][o] = x[row][src[o]] names the element (tail tile, p2v gather) it was read from; bf16 and fp32x3."""
    rows, m = 389, _pooled_rows(389)
    for wide in (False, True):
        p = R.position_code(5, rows, 32 if gather else 64, 32, 32 if gather else 0, m, wide=wide)
        z64, z32, zb = torch.zeros((32, 64), dtype=I64), torch.zeros((32, 32), dtype=I64), torch.zeros((32,), dtype=I64)
        x = R.cat_rows(p['xa'], p['xb'], p['b_index'])
        want = R.pfn_forward(x, z64, zb, p['w'], z32, zb, bf16=not wide)['out']
        gws = [_f(t) for t in (z64, zb, p['w'], z32, zb)]
        if wide:
            a, b_ = _f(p['xa']), _f(p['xb'])
            out = native.pfn_block_split_forward(a, _amax(a), b_, None if b_ is None else _amax(b_), _i32(p['b_index']), *gws)[0]
        else:
            out = native.pfn_block_forward(_up(p['xa'], BF16), _up(p['xb'], BF16), _i32(p['b_index']), *gws)[0]
        _same(out, want, F32 if wide else BF16, 'pfn position %s' % ('x3' if wide else 'bf16'), _explainer(p, wide))


# =========================================================================================================================================
# NaN masks: `mask > 0` keeps -- a NaN mask drops, at every mask of every row entry point (include/pcacc.h)
# =========================================================================================================================================
@gpu
@pytest.mark.parametrize('k,n', [(32, 32), (64, 128), (128, 128)])
def test_nan_masks_drop_on_the_matrix_core_paths(k, n):
    for mode in ('bf16', 'x3'):
        _forward_case(mode, k, n, 129, nan=True)
        _cat_case(mode, k, n, 129, nan=True)
        _wgrad_case(mode, k, n, 129, nan=True)


@gpu
def test_nan_masks_drop_on_the_fp32_paths():
    for k, n in ((32, 33), (128, 100), (9, 64), (64, 2)):
        _fp32_forward(k, n, 129, nan=True)
        _fp32_forward(k, n, 129, (BF16,) * 5, nan=True)
    for k, n in ((32, 32), (128, 128), (9, 64), (64, 2)):
        _fp32_wgrad(k, n, 129, nan=True)
        _fp32_wgrad(k, n, 129, (BF16, BF16, F32), nan=True)


# =========================================================================================================================================
# the autograd paths: ops.linear_rows, ResnetBlockFC.forward_pooled, ops.pfn_block(pool=True) in the bf16, fp32x3 and mixed modes
# =========================================================================================================================================
@pytest.fixture
def compute_mode():
    """set(mode): 'bf16' | 'fp32x3' | 'mixed' for the operators issued afterwards; fp32 defaults restored (and the twin registry emptied) afterwards."""
    def set_(mode):
        ops.set_split(mode in ('fp32x3', 'mixed'))
        ops.set_mixed(mode == 'mixed')
    yield set_
    ops.set_mixed(False)
    ops.set_split(False)


def _rows_in(t, mode, grad=True):
    """An int64 row tensor as the mode's chains hold it: bf16 leaf, fp32 leaf, or the bf16 shadow of an fp32 twin."""
    if mode == 'bf16':
        return _up(t, BF16).requires_grad_(grad)
    if mode == 'fp32x3':
        return _f(t).requires_grad_(grad)
    return ops.shadow(_f(t)).requires_grad_(grad)


def _linear_layer(w, b):
    layer = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None).to(_dev())
    with torch.no_grad():
        layer.weight.copy_(_f(w))
        if b is not None:
            layer.bias.copy_(_f(b))
    return layer


AUTOGRAD_ROWS = 2048 + 129                                       # at least ops.MIN_ROWS_FUSED_LINEAR, a partial last tile


@gpu
@pytest.mark.parametrize('k,n', [(64, 32), (128, 128)])
@pytest.mark.parametrize('mode', ['bf16', 'fp32x3', 'mixed'])
def test_linear_rows_autograd(mode, k, n, compute_mode):
    """y, d x, d W, d bias and d residual of ops.linear_rows(pre-ReLU, post-ReLU, residual).  The gradient kernels of the mixed mode are the bf16 ones;
    its forward is the fp32x3 one, with the shadow y16 = RNE(y)."""
    compute_mode(mode)
    rows, sd = AUTOGRAD_ROWS, _seed(k, n, 29)
    f = R.dense_small(sd, rows, k, n, wmax=2)
    x, w, b, res = f['x'], f['w'], f['bias'], f['residual']
    gy = R.small_grad(sd + 1, (rows, n), -31, 31)                 # wide enough for d x to pass 256, where bf16 rounds
    half = mode != 'fp32x3'                                       # gradients (and in bf16 mode values) are bf16 rows
    dt = BF16 if half else F32
    layer = _linear_layer(w, b)
    xg, rg = _rows_in(x, mode), _rows_in(res, mode)
    y = ops.linear_rows(xg, layer, pre_relu=True, post_relu=True, residual=rg)
    y.backward(_up(gy, dt))
    want_y = R.linear(x, w, b, res, True, True, bf16=mode == 'bf16')
    _same(y, want_y, dt, mode + ' y')
    if mode == 'mixed':
        _same(ops.twin(y.detach()), want_y, F32, 'mixed y, fp32 twin')
    y_seen = R.round_bf16(want_y) if mode == 'mixed' else want_y  # the mask the backward reads
    _same(xg.grad, R.linear(gy, w.t().contiguous(), in_mask=y_seen, out_mask=x, bf16=half), dt, mode + ' d x')
    dw, db = R.split_layout(R.wgrad_aug(gy, x, y_seen, True))
    _same(layer.weight.grad, dw, F32, mode + ' d W')
    _same(layer.bias.grad, db, F32, mode + ' d bias')
    _same(rg.grad, gy * (y_seen > 0), dt, mode + ' d residual')
    assert sum(R.bf16_rounding_census(R.linear(gy, w.t().contiguous(), in_mask=y_seen, out_mask=x))) > 0, 'no tie and no inexact bf16 value in d x: the rounding is not exercised'


def _pool_reference(xa, p2v, m):
    """segment max over each pillar's points and the winner (lowest point index attaining the maximum) per (pillar, channel); -1 for an empty pillar."""
    rows, c = xa.shape
    seg = p2v.long().view(-1, 1).expand(-1, c)
    pooled = torch.full((m, c), -(1 << 40), dtype=I64).scatter_reduce(0, seg, xa, 'amax')
    cand = torch.where(xa == pooled[p2v.long()], torch.arange(rows).view(-1, 1).expand(-1, c), torch.full_like(xa, rows))
    win = torch.full((m, c), rows, dtype=I64).scatter_reduce(0, seg, cand, 'amin')
    return pooled, torch.where(win == rows, torch.full_like(win, -1), win)


@gpu
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('mode', ['bf16', 'fp32x3', 'mixed'])
def test_pfn_block_autograd(mode, pool, compute_mode):
    """ResnetBlockFC.forward_pooled (pool = False: pooled rows are an input with their own gradient, summed over each pillar's points) and
    ops.pfn_block(pool=True) (pooled = segment max of x inside the node: the pooled gradient goes to each (pillar, channel)'s winner, added to d x).
    Output, d x, d pooled and all five parameter gradients.  Per-pillar sums are fp32 sums of integers, stored once in the rows' type."""
    from pcaccumulation_amd.pillar_encoder import ResnetBlockFC
    compute_mode(mode)
    rows, m, sd = AUTOGRAD_ROWS, 300, _seed(pool, 31)
    half = mode != 'fp32x3'
    dt = BF16 if half else F32
    xa, pooled_in, p2v = R.pfn_inputs(sd, rows, m)
    p2v[:m] = torch.arange(m, dtype=torch.int32)                   # every pillar owns a point
    wts = R.pfn_weights(sd + 1)
    w0, b0, ws, w1, b1 = wts
    gout = R.small_grad(sd + 2, (rows, 32))
    blk = ResnetBlockFC(64, 32).to(_dev())
    with torch.no_grad():
        for p, v in ((blk.fc_0.weight, w0), (blk.fc_0.bias, b0), (blk.shortcut.weight, ws), (blk.fc_1.weight, w1), (blk.fc_1.bias, b1)):
            p.copy_(_f(v))
    pidx = ops.PillarIndex.from_point_map(p2v.to(_dev()), m)
    xg = _rows_in(xa, mode)
    if pool:
        pooled, win = _pool_reference(xa, p2v, m)
        assert ops.pfn_pool_block_available(blk, xg, pidx)
        out = ops.pfn_block(blk, xg, None, pidx, pool=True)
    else:
        pooled, pg = pooled_in, _rows_in(pooled_in, mode)
        assert ops.pfn_block_available(blk, xg, pg)
        out = blk.forward_pooled(xg, pg, pidx)
    out.backward(_up(gout, dt))
    x = R.cat_rows(xa, pooled, p2v)
    fwd = R.pfn_forward(x, *wts, bf16=mode == 'bf16')
    _same(out, fwd['out'], dt, mode + ' out')
    if mode == 'mixed':
        _same(ops.twin(out.detach()), fwd['out'], F32, 'mixed out, fp32 twin')
    hr_seen = R.round_bf16(fwd['relu_h']) if mode == 'mixed' else fwd['relu_h']            # hr16 is what the bf16 backward of the mixed mode reads
    bwd = R.pfn_backward(x, hr_seen, gout, w0, ws, w1, bf16=half)
    gxa, gxb = bwd['grad_x'][:, :32], bwd['grad_x'][:, 32:]
    gpool = torch.zeros((m, 32), dtype=I64).index_add_(0, p2v.long(), gxb)
    if half:
        gpool = R.round_bf16(gpool)
    if pool:
        add = torch.zeros_like(gxa).contiguous()
        cols = torch.arange(32).view(1, -1).expand(m, -1)
        add[win.view(-1), cols.reshape(-1)] = gpool.view(-1)       # one winner per (pillar, channel): no two writes meet
        gxa = gxa + add
        if half:
            gxa = R.round_bf16(gxa)
    else:
        _same(pg.grad, gpool, dt, mode + ' d pooled')
    _same(xg.grad, gxa.contiguous(), dt, mode + ' d x')
    for name, p in (('w1', blk.fc_1.weight), ('b1', blk.fc_1.bias), ('ws', blk.shortcut.weight), ('w0', blk.fc_0.weight), ('b0', blk.fc_0.bias)):
        lo, hi, shape = native.PFN_BLOCK_SLICES[name]
        _same(p.grad, bwd['params'][lo:hi].view(shape), F32, mode + ' d ' + name)
