"""Exact integer references and input families for the per-point linear layers and the fused PFN block (tests/test_rows_exact.py).  No GPU
dependency.

On small-integer operands every product and every partial sum of a row-linear layer is an integer below 2^24, which bf16 products, the fp16
hi / lo halves of fp32x3 (power-of-two scales), fp32 FMAs and the fp32 MFMA all represent exactly: summation order, partial slots, atomics and
the MFMA layout cannot change a bit, and a kernel's result must equal the integer result at EVERY element.  A bf16 value appears exactly where a
kernel holds one -- the places include/pcacc.h names -- and is the exact value rounded once, to nearest even, at each of them:
    y of the bf16 layers (with a residual: y = bf16(bf16(x w^T + bias) + residual), the result tile is a bf16 tile before the residual is added),
    y16 / out16 / hr16 of the 'mixed' mode, relu_h and out of the bf16 PFN block, d(h) inside the bf16 PFN backward, the bf16 gradients.

Everything is torch.int64 on the CPU until `exact_f32` / `exact_bf16` (conv_exact_reference.py); masks may also be float tensors (their edge
values -0.0, the smallest normal and NaN are not integers) -- the one rule everywhere is `mask > 0` keeps, so a NaN mask drops.  Matrix products
run as float64 matmul after the generator has proven |a|max |b|max k < 2^53 (every partial sum then is an exactly represented integer), and
every reference function also runs on the absolute values of its operands and refuses an input whose sum |term| reaches 2^24."""
import math

import torch

from conv_exact_reference import (I64, LIMIT, NotExact, _bound, _gen, _randint, _sparse_signs, bf16_rounding_census, exact_bf16, exact_f32,  # noqa: F401
                                  rounded_bf16)

TINY = 1.1754943508222875e-38                                   # the smallest positive normal fp32 (and bf16) value, 2^-126
MASK_EDGES = (-1.0, -0.0, 0.0, TINY, 1.0)


# ---- building blocks ----------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """Integer matrix product a [m,k] @ b [k,n] -> int64, as a float64 matmul: with k |a|max |b|max < 2^53 every partial sum, in any order, is an
    integer float64 represents exactly."""
    assert a.dtype == I64 and b.dtype == I64 and a.shape[1] == b.shape[0]
    if a.numel() == 0 or b.numel() == 0:
        return torch.zeros((a.shape[0], b.shape[1]), dtype=I64)
    assert a.shape[1] * int(a.abs().max()) * int(b.abs().max()) < (1 << 53), 'float64 matmul would not be exact'
    return (a.double() @ b.double()).to(I64)


def keep(mask):
    """The mask rule of every row entry point: an element counts where mask > 0.  -1, -0.0, +0.0 and NaN drop; 2^-126 and 1 keep."""
    return mask > 0


def _masked(t, mask):
    return t if mask is None else torch.where(keep(mask), t, torch.zeros_like(t))


def round_bf16(t):
    """int64 -> the integer a bf16 store keeps of it (round to nearest even); below 2^24 a bf16 value is an integer again."""
    return rounded_bf16(t).to(I64)


def bf16_weights(w):
    """fp32 integer weights as a bf16 kernel uses them: 'rounded to bf16 once per launch', to nearest even (257 -> 256, 259 -> 260)."""
    return round_bf16(w)


def cat_rows(xa, xb=None, b_index=None):
    """The two-piece row: cat(xa[row], xb[b_index[row]]); b_index None: xb[row]; xb None: xa."""
    if xb is None:
        return xa
    return torch.cat([xa, xb if b_index is None else xb[b_index.long()]], dim=1)


# ---- the operations ------------------------------------------------------------------------------------------------------------------------------
def linear(x, w, bias=None, residual=None, pre_relu=False, post_relu=False, in_mask=None, out_mask=None, bf16=False):
    """y = post(pre(x) @ w^T + bias + residual), x [rows,k], w [n,k]: pre = ReLU (pre_relu) then in_mask, post = ReLU (post_relu) then out_mask.
    bf16: the values of the bf16 kernel -- x w^T + bias rounded to bf16, then the residual added and the sum rounded again."""
    xe = _masked(x.clamp_min(0) if pre_relu else x, in_mask)
    y = _mm(xe, w.t().contiguous())
    ab = _mm(xe.abs(), w.abs().t().contiguous())
    if bias is not None:
        y, ab = y + bias, ab + bias.abs()
    if bf16:
        _bound('linear', ab)
        y = round_bf16(y)
        ab = y.abs()
    if residual is not None:
        y, ab = y + residual, ab + residual.abs()
    _bound('linear', ab)
    if bf16 and residual is not None:
        y = round_bf16(y)
    if post_relu:
        y = y.clamp_min(0)
    return _masked(y, out_mask)


def linear_cat_backward(gy, w_t, na, dy_mask=None, out_mask_a=None, out_mask_b=None, b_index=None, bf16=False):
    """The backward-data form of the cat entry points: (gy masked where dy_mask <= 0) @ w_t^T with w_t = W^T [k,n], the [rows,k] result split at
    column na into (y, y2) and masked by cat(out_mask_a[row], out_mask_b[b_index[row]])."""
    om = None if out_mask_a is None else cat_rows(out_mask_a, out_mask_b, b_index)
    y = linear(gy, w_t, in_mask=dy_mask, out_mask=om, bf16=bf16)
    return y[:, :na].contiguous(), y[:, na:].contiguous()


def wgrad_aug(dy, x, dy_mask=None, x_relu=False):
    """dw_aug [n,k+1] = dYeff^T @ [Xeff | 1]: dYeff = dy where dy_mask > 0, Xeff = relu(x) when x_relu; column k is the bias gradient."""
    g = _masked(dy, dy_mask)
    xe = torch.cat([x.clamp_min(0) if x_relu else x, torch.ones((x.shape[0], 1), dtype=I64)], dim=1)
    _bound('wgrad_aug', _mm(g.abs().t().contiguous(), xe.abs()))
    return _mm(g.t().contiguous(), xe)


def split_layout(aug):
    """[n,k+1] rows -> (dW [n,k], db [n]), the second result layout (dW followed by db, each contiguous)."""
    return aug[:, :-1].contiguous(), aug[:, -1].contiguous()


PFN_ORDER = (('w1', (32, 32)), ('b1', (32,)), ('ws', (32, 64)), ('w0', (32, 64)), ('b0', (32,)))       # grad_params [5184], include/pcacc.h


def pfn_forward(x, w0, b0, ws, w1, b1, bf16=False):
    """ResnetBlockFC 64 -> 32 -> 32 with the linear shortcut: h = relu(x) w0^T + b0, out = relu(h) w1^T + b1 + x ws^T.
    -> dict(out, relu_h, xmask (bit c: x[row][c] > 0, as int64 two's complement of the u64), hmask (bit c: h[row][c] > 0)).
    bf16: relu_h is the bf16 the kernel stores (and multiplies with), out is rounded once."""
    hr = linear(x, w0, b0, pre_relu=True).clamp_min(0)
    if bf16:
        hr = round_bf16(hr)
    o = _mm(hr, w1.t().contiguous()) + _mm(x, ws.t().contiguous())
    ab = _mm(hr, w1.abs().t().contiguous()) + _mm(x.abs(), ws.abs().t().contiguous())
    if b1 is not None:
        o, ab = o + b1, ab + b1.abs()
    _bound('pfn_forward', ab)
    xbits = (x > 0).to(I64)
    lo = (xbits[:, :63] << torch.arange(63, dtype=I64)).sum(1)
    xmask = torch.where(xbits[:, 63] > 0, lo - (1 << 62) - (1 << 62), lo)                    # bit 63 set: the negative int64 with the same bits
    hmask = ((hr > 0).to(I64) << torch.arange(32, dtype=I64)).sum(1)
    return {'out': round_bf16(o) if bf16 else o, 'relu_h': hr, 'xmask': xmask, 'hmask': hmask}


def pfn_backward(x, relu_h, gout, w0, ws, w1, bf16=False):
    """d(h) = (gout @ w1) where relu_h > 0;  d(x) = (d(h) @ w0) where x > 0, + gout @ ws;  parameter gradients in the header's order.
    bf16: d(h) is held as bf16 between the two products (and in the fc_0 gradients), d(x) is rounded once; the parameter gradients are fp32.
    -> dict(grad_x [rows,64], grad_h, params [5184])."""
    dh = _masked(linear(gout, w1.t().contiguous()), relu_h)
    if bf16:
        dh = round_bf16(dh)
    a = _masked(linear(dh, w0.t().contiguous()), x)
    b = linear(gout, ws.t().contiguous())
    _bound('pfn_backward d(x)', a.abs() + b.abs())
    gx = a + b
    dw1 = wgrad_aug(gout, relu_h)
    dws = wgrad_aug(gout, x)
    dw0 = wgrad_aug(dh, x, x_relu=True)
    params = torch.cat([dw1[:, :-1].reshape(-1), dw1[:, -1], dws[:, :-1].reshape(-1), dw0[:, :-1].reshape(-1), dw0[:, -1]])
    return {'grad_x': round_bf16(gx) if bf16 else gx, 'grad_h': dh, 'params': params}


# ---- the fp32x3 split, simulated ------------------------------------------------------------------------------------------------------------------
def split_scale(amax):
    """The power of two that puts amax into [2^13, 2^14) (1 for amax = 0)."""
    return 1.0 if amax == 0 else 2.0 ** (14 - math.frexp(float(amax))[1])


def split_halves(t, amax=None):
    """int64 -> (hi, lo) as float64 tensors in units of the operand: hi = fp16(s v) / s, lo = fp16(s v - hi) / s with s = split_scale(amax or
    max|t|); asserts hi + lo == v exactly (the split itself loses nothing)."""
    f = exact_f32(t)
    s = split_scale(float(f.abs().max()) if amax is None else amax)
    hi = (f * s).to(torch.float16)
    lo = (f * s - hi.float()).to(torch.float16)
    assert torch.equal(hi.float() + lo.float(), f * s), 'hi + lo does not carry the operand exactly'
    return hi.double() / s, lo.double() / s


def lo_count(t, amax=None):
    return int((split_halves(t, amax)[1] != 0).sum()) if t.numel() else 0


def assert_one_lo_per_product(x, w, x_amax=None, per_row_w=True):
    """fp32x3 forms w_hi x_hi + w_hi x_lo + w_lo x_hi and never w_lo x_lo: no product of x [rows,k] @ w [n,k]^T may need both lo halves."""
    xl = split_halves(x, x_amax)[1] != 0
    if per_row_w:
        wl = torch.stack([split_halves(w[o])[1] != 0 for o in range(w.shape[0])])
    else:
        wl = split_halves(w)[1] != 0
    both = xl.double() @ wl.double().t()
    assert float(both.max()) == 0.0 if both.numel() else True, 'a product needs the lo halves of both factors'


# ---- input families (seeded, deterministic); every one asserts its own conditions ----------------------------------------------------------------------
def gather_index(seed, rows, m):
    """b_index [rows] into a pooled table of m rows: repeats, the first and the last pooled row, not monotone (asserted from 4 rows on)."""
    g = _gen(seed)
    idx = torch.randint(0, m, (rows,), generator=g)
    idx[0] = m - 1
    if rows >= 2:
        idx[-1] = 0
    if rows >= 4:
        idx[1], idx[2] = 0, m - 1                                # last, first, last ... first: down, up, repeats
        d = idx[1:] - idx[:-1]
        assert bool((d > 0).any()) and bool((d < 0).any()), 'gather_index: monotone'
        assert len(set(idx.tolist())) < rows and int(idx.min()) == 0 and int(idx.max()) == m - 1
    return idx.to(torch.int32)


def dense_small(seed, rows, k, n, lo=-3, hi=3, wmax=1):
    """Family 1: x uniform in {lo..hi}, w in {-wmax..wmax}, bias and residual in {-4..4}.  -> dict(x, w, bias, residual)."""
    g = _gen(seed)
    f = {'x': _randint(g, lo, hi, (rows, k)), 'w': _randint(g, -wmax, wmax, (n, k)), 'bias': _randint(g, -4, 4, (n,)),
         'residual': _randint(g, -4, 4, (rows, n))}
    linear(f['x'], f['w'], f['bias'], f['residual'])
    return f


def position_value(piece, row, col, wide):
    """The value that names element (piece, row, col).  wide (fp32 / fp32x3 rows): 1 + col + 128 (row mod 8191) + 2^20 piece, decodable, up to 21
    bits (the fp32x3 lo half is in use).  Otherwise (bf16 rows): a hash in 1..255, unrelated between neighbours in any direction."""
    if wide:
        return 1 + col + 128 * (row % 8191) + (piece << 20)
    v = (row * 7919 + col * 104729 + piece * 1299709 + 12345) % 2147483647
    v = (v * 48271) % 2147483647
    return (v >> 7) % 255 + 1


def position_code(seed, rows, ka, n, kb=0, m=0, wide=False):
    """Family 2: one-hot weights -- output o reads input column src[o] of the (concatenated) row -- and activations that name their own
    (piece, row, column).  kb > 0: a second piece xb [m, kb] read through b_index.  -> dict(xa, xb, b_index, w, src)."""
    k = ka + kb
    r = torch.arange(rows, dtype=I64).view(-1, 1)
    f = {'xa': position_value(0, r, torch.arange(ka, dtype=I64).view(1, -1), wide), 'xb': None, 'b_index': None}
    if kb:
        f['xb'] = position_value(1, torch.arange(m, dtype=I64).view(-1, 1), torch.arange(kb, dtype=I64).view(1, -1), wide)
        f['b_index'] = gather_index(seed, rows, m)
    src = (torch.arange(n, dtype=I64) * 5 + 3 + int(seed)) % k
    w = torch.zeros((n, k), dtype=I64)
    w[torch.arange(n), src] = 1
    f['w'], f['src'] = w, src
    assert bool((w.sum(1) == 1).all()) and int(w.abs().sum()) == n
    if kb and n >= 8:
        assert bool((src < ka).any()) and bool((src >= ka).any()), 'position_code: one piece is never read'
    return f


def explain_position(f, where, got, wide=False, transposed_na=None):
    """For a mismatch of a position-code forward at where = (row, o): the element that should have been read and -- if one exists nearby -- the
    element that holds the value the kernel gave (a neighbouring row, the neighbouring pooled row, the other piece, a column 8 away)."""
    row, o = where
    ka = f['xa'].shape[1]
    c = int(f['src'][o])
    if c < ka or f['xb'] is None:
        piece, prow, col = 0, row, c
    else:
        piece, prow, col = 1, (int(f['b_index'][row]) if f['b_index'] is not None else row), c - ka
    msg = 'output (row %d, col %d) reads piece %d (row %d, col %d)' % (row, o, piece, prow, col)
    if got != got or got != int(got):
        return msg + '; the kernel gave %r, which no input element holds' % (got,)
    got = int(got)
    if got == 0:
        return msg + '; the kernel gave 0'
    for p, t in ((0, f['xa']), (1, f['xb'])):
        if t is None:
            continue
        base = row if p == 0 else (int(f['b_index'][row]) if f['b_index'] is not None else row)
        cands = [base + d for d in (0, -1, 1, -2, 2)] + [base ^ 1] + ([row] if p == 1 else [])
        for rr in cands:
            if not 0 <= rr < t.shape[0]:
                continue
            hit = (t[rr] == got).nonzero()
            if hit.numel() and (p, rr, int(hit[0])) != (piece, prow, col):
                return msg + '; the kernel gave %d = piece %d (row %d, col %d)' % (got, p, rr, int(hit[0]))
    return msg + '; the kernel gave %d, found in no neighbouring row of either piece' % got


def lo_activations(seed, rows, k, n, bits=20, per_row=8, one_large=False):
    """Family 3a: 20-bit activations (hi and lo halves both in use), weights in {-1,0,1} at `per_row` places of each output: only w_hi x_lo
    carries the lo plane.  one_large: element (rows // 2, 1) alone is 20 bits wide and fixes the tensor scale (it needs its lo half), the rest are
    odd values below 2^9 that sit 2^11 below it after scaling: they must survive a scale another row's element chose."""
    g = _gen(seed)
    top = (1 << bits) - 1
    if one_large:
        x = _randint(g, -511, 511, (rows, k)) | 1
        x[rows // 2, 1] = top
    else:
        x = _randint(g, -top, top, (rows, k))
        x[0, 0] = top
    w = _sparse_signs(g, (n, k), per_row)
    linear(x, w)
    if not one_large:
        assert lo_count(x) > 0, 'lo_activations: every lo half is zero'
    assert lo_count(w) == 0
    assert_one_lo_per_product(x, w)
    return {'x': x, 'w': w, 'bias': None, 'residual': None}


def lo_weights(seed, rows, k, n, per_row=6):
    """Family 3b: 18- to 20-bit odd weights at `per_row` places of each output row (the weight scale is per row), activations in {-1,0,1}:
    only w_lo x_hi carries the lo plane."""
    g = _gen(seed)
    x = _randint(g, -1, 1, (rows, k))
    w = torch.zeros((n, k), dtype=I64)
    idx = torch.randint(0, k, (n, per_row), generator=g)
    mag = _randint(g, 1 << 17, (1 << 20) - 1, (n, per_row)) | 1
    w.scatter_(1, idx, mag * (_randint(g, 0, 1, (n, per_row)) * 2 - 1))
    linear(x, w)
    assert sum(lo_count(w[o]) for o in range(n)) > 0 and lo_count(x) == 0
    assert_one_lo_per_product(x, w)
    return {'x': x, 'w': w, 'bias': None, 'residual': None}


def lo_pieces(seed, rows, ka, kb, m, n):
    """Family 3, two-piece rows: the pooled piece is about 2^10 larger than the point piece (pooled up to 2^19, points below 2^9); the
    kernel must scale both with the LARGER maximum -- with the point piece's own scale the pooled values overflow fp16."""
    g = _gen(seed)
    xa = _randint(g, -511, 511, (rows, ka)) | 1
    xb = _randint(g, -(1 << 19) + 1, (1 << 19) - 1, (m, kb))
    xb[m - 1, 0] = (1 << 19) - 1
    idx = gather_index(seed, rows, m)
    w = _sparse_signs(g, (n, ka + kb), 8)
    x = cat_rows(xa, xb, idx)
    linear(x, w)
    amax = float(max(int(xa.abs().max()), int(xb.abs().max())))
    assert int(xb.abs().max()) >= 512 * int(xa.abs().max())
    assert lo_count(xb, amax) > 0
    split_halves(xa, amax)
    return {'xa': xa, 'xb': xb, 'b_index': idx, 'w': w}


def bf16_mantissa(seed, rows, k, n, per_row=16):
    """Family 4: activations with all 8 significant bits of bf16 in use (|x| <= 255, odd values in every row), weights sparse in {-1,0,1}."""
    g = _gen(seed)
    x = _randint(g, -255, 255, (rows, k))
    x[:, 0] |= 1
    x[0, 1] = 255
    w = _sparse_signs(g, (n, k), per_row)
    f = {'x': x, 'w': w, 'bias': _randint(g, -4, 4, (n,)), 'residual': None}
    linear(x, w, f['bias'])
    exact_bf16(x)
    assert int(x.abs().max()) == 255 and bool((x % 2 != 0).any())
    return f


def bf16_ties(seed, rows, k, n):
    """Family 5: exact results halfway between two bf16 values, with the even neighbour below (round down) and above (round up): one-hot weights,
    x in 1..255, bias 256 -> results in 257..511, where bf16 neighbours are 2 apart and every odd value is a tie."""
    g = _gen(seed)
    x = _randint(g, 1, 255, (rows, k))
    x[0, :4] = torch.tensor([1, 3, 2, 255])                                              # 257 -> 256 (down), 259 -> 260 (up), 258 exact, 511 -> 512
    src = (torch.arange(n, dtype=I64) * 5 + int(seed)) % k
    src[:4] = torch.arange(4)[:n]
    w = torch.zeros((n, k), dtype=I64)
    w[torch.arange(n), src] = 1
    bias = torch.full((n,), 256, dtype=I64)
    y = linear(x, w, bias)
    ties, _ = bf16_rounding_census(y)
    odd = y[y % 2 == 1]
    down, up = int(((odd >> 1) % 2 == 0).sum()), int(((odd >> 1) % 2 == 1).sum())
    assert ties == odd.numel() and down > 0 and up > 0, 'bf16_ties: ties %d, down %d, up %d' % (ties, down, up)
    return {'x': x, 'w': w, 'bias': bias, 'residual': None}


def weight_rounding(seed, rows, k, n):
    """Family 6: fp32 integer weights bf16 cannot hold (257, 259, 261, 511, -385 ...) at 4 places of each output row, x in {-1,0,1}: the bf16 kernels
    use bf16_weights(w), every other kernel uses w itself."""
    g = _gen(seed)
    x = _randint(g, -1, 1, (rows, k))
    w = torch.zeros((n, k), dtype=I64)
    idx = torch.randint(0, k, (n, 4), generator=g)
    mag = _randint(g, 128, 255, (n, 4)) * 2 + 1
    w.scatter_(1, idx, mag * (_randint(g, 0, 1, (n, 4)) * 2 - 1))
    w[0, :4] = torch.tensor([257, 259, 261, -511])
    assert int((bf16_weights(w) != w).sum()) > 0
    assert bf16_weights(torch.tensor([257, 259, 261, -511])).tolist() == [256, 260, 260, -512]
    linear(x, w)
    linear(x, bf16_weights(w))
    return {'x': x, 'w': w, 'bias': None, 'residual': None}


def mask_edges(seed, shape, nan=False):
    """Family 7: a float mask drawn from {-1, -0.0, +0.0, 2^-126, 1} (nan: NaN too), every value present from 16 elements on."""
    g = _gen(seed)
    vals = torch.tensor(MASK_EDGES + ((float('nan'),) if nan else ()), dtype=torch.float32)
    m = vals[torch.randint(0, vals.numel(), tuple(shape), generator=g)]
    flat = m.view(-1)
    if flat.numel() >= 16:
        flat[:vals.numel()] = vals
        assert bool(torch.signbit(flat[1])) and float(flat[1]) == 0.0 and not bool(torch.signbit(flat[2]))
    assert m.to(torch.bfloat16).float().equal(m) or nan                                   # every edge value is a bf16 value too
    return m


def relu_edges(seed, shape):
    """Forward inputs under a ReLU: {-1, -0.0, +0.0, 1} as a float tensor and the same as int64 (both zeros are 0).  The smallest normal is a mask
    value only: 2^-126 times a weight is no integer, and the fp32x3 split flushes it."""
    g = _gen(seed)
    vals = torch.tensor((-1.0, -0.0, 0.0, 1.0), dtype=torch.float32)
    x = vals[torch.randint(0, 4, tuple(shape), generator=g)]
    if x.numel() >= 4:
        x.view(-1)[:4] = vals
    return x, x.to(I64)


def small_grad(seed, shape, lo=-3, hi=3):
    return _randint(_gen(seed), lo, hi, shape)


def relu_like_mask(seed, shape):
    """A mask as a ReLU output is: about half zeros, the rest positive; a few negatives to tell `<= 0` from `== 0` and `< 0`."""
    m = _randint(_gen(seed), -1, 3, shape)
    return torch.where(m == 2, torch.zeros_like(m), m)


def pfn_weights(seed, wmax=2, sparse1=0):
    """(w0 [32,64], b0, ws [32,64], w1 [32,32], b1) small integers; sparse1 > 0: w1 in {-1,0,1} at that many places per row."""
    g = _gen(seed)
    w1 = _sparse_signs(g, (32, 32), sparse1) if sparse1 else _randint(g, -wmax, wmax, (32, 32))
    return (_randint(g, -wmax, wmax, (32, 64)), _randint(g, -4, 4, (32,)), _randint(g, -wmax, wmax, (32, 64)), w1, _randint(g, -4, 4, (32,)))


def pfn_inputs(seed, rows, m=0, lo=-3, hi=3):
    """x of a PFN block: [rows,64] (m = 0) or (xa [rows,32], pooled [m,32], p2v); values uniform in {lo..hi}."""
    g = _gen(seed)
    if not m:
        return _randint(g, lo, hi, (rows, 64)), None, None
    return _randint(g, lo, hi, (rows, 32)), _randint(g, lo, hi, (m, 32)), gather_index(seed, rows, m)


def pfn_wide_h(seed, rows):
    """PFN block, fp32x3: the variant in which h ITSELF needs its lo half -- x in 8 bits (no lo half), w0 in {-3..3}: h up to 64 * 255 * 3 < 2^16 with
    its low bits in use, beyond the 11 bits of the hi half of the per-wave scale; w1 sparse in {-1,0,1} so that relu(h) w1^T stays below 2^24."""
    g = _gen(seed)
    x = _randint(g, -255, 255, (rows, 64))
    w0, b0, ws, _, b1 = pfn_weights(seed, 3)
    w1 = _sparse_signs(g, (32, 32), 6)
    r = pfn_forward(x, w0, b0, ws, w1, b1)
    assert lo_count(r['relu_h']) > 0 and lo_count(x) == 0, 'pfn_wide_h: relu(h) fits its hi half'
    return x, (w0, b0, ws, w1, b1)
