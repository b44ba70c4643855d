"""Exact integer references and input families for the convolution kernels (tests/test_conv_exact.py).  No GPU dependency.

On small-integer operands every product and every partial sum of a convolution is an integer below 2^24, which bf16 products, the fp16 hi / lo
halves of fp32x3 (power-of-two scales) and fp32 FMAs all represent exactly: summation order, atomics, split-K slots and the MFMA layout cannot
change a bit, and a kernel's result must equal the int64 result at EVERY element (rounded once, to nearest even, where the output is bf16).

Layouts are the kernels': activations channels-last rows [n_img, h, w, c]; 3x3 weights [c_out, c_in, 3, 3], 3x3x3 weights [c_out, c_in, 3, 3, 3]
(frame tap first), transposed 2x2 weights [c_in, c_up, 2, 2].  Everything is torch.int64 on the CPU until `exact_f32`.

Every reference function also runs on the absolute values of its operands and asserts `sum |term| < 2^24` for every output element (bias
included): an input that violates it is a bug in the test, never a tolerance to widen."""
import torch
import torch.nn.functional as F

LIMIT = 1 << 24
I64 = torch.int64


class NotExact(AssertionError):
    pass


def _i64(t):
    assert t is None or (t.dtype == I64 and t.device.type == 'cpu'), 'int64 CPU tensors only'
    return t


def _bound(name, abs_sum):
    worst = int(abs_sum.max()) if abs_sum.numel() else 0
    if worst >= LIMIT:
        raise NotExact('%s: sum |term| reaches %d >= 2^24 -- the family is not exact' % (name, worst))
    return worst


# ---- the operations, in int64 ----------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """Integer matrix product a [m,k] @ b [k,n] -> int64.  Where k * max|a| * max|b| < 2^31 no partial sum can leave int32, and the product runs in
    int32 (four times faster on the CPU) before it is widened: integer arithmetic either way, the same result bit for bit."""
    if a.numel() == 0 or b.numel() == 0:
        return torch.zeros((a.shape[0], b.shape[1]), dtype=I64)
    if a.shape[1] * int(a.abs().max()) * int(b.abs().max()) < (1 << 31):
        return (a.to(torch.int32) @ b.to(torch.int32)).to(I64)
    return a @ b


def _patches(x):
    """x [n,h,w,c] -> [n*h*w, 9*c]: the 3x3 neighbourhood of every pixel (zero outside the image), taps in (dy, dx) order, channels fastest."""
    n, h, ww, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.cat([xp[:, dy:dy + h, dx:dx + ww] for dy in range(3) for dx in range(3)], dim=3).reshape(n * h * ww, 9 * c)


def _conv2_raw(x, w):
    """x [n,h,w,ci], w [co,ci,3,3] -> [n,h,w,co]: out[y,x,o] = sum x[y+dy-1, x+dx-1, c] w[o,c,dy,dx], zero outside the image."""
    n, h, ww, ci = x.shape
    co = w.shape[0]
    return _mm(_patches(x), w.permute(2, 3, 1, 0).reshape(9 * ci, co)).view(n, h, ww, co)


def _conv_raw(x, w, frames):
    """kt = 1: _conv2_raw.  kt = 3: frame t of a sample reads frames t-1, t, t+1 OF THE SAME SAMPLE (zero outside it)."""
    if w.dim() == 4:
        return _conv2_raw(x, w)
    n, h, ww, ci = x.shape
    assert n % frames == 0
    x5 = x.view(n // frames, frames, h, ww, ci)
    out = torch.zeros((n // frames, frames, h, ww, w.shape[0]), dtype=I64)
    for dt in range(3):
        lo, hi = max(0, 1 - dt), min(frames, frames + 1 - dt)          # output frames t with 0 <= t + dt - 1 < frames
        if lo < hi:
            src = x5[:, lo + dt - 1:hi + dt - 1].reshape(-1, h, ww, ci)
            out[:, lo:hi] += _conv2_raw(src, w[:, :, dt]).view(n // frames, hi - lo, h, ww, -1)
    return out.view(n, h, ww, -1)


def conv3x3(x, w, bias=None, frames=1, relu=False, mask=None, out_mask=None):
    """3x3 (w [co,ci,3,3]) / 3x3x3 (w [co,ci,3,3,3]) convolution, padding 1.  mask (shape of x): elements of x where mask <= 0 are read as
    zero (`mask > 0` keeps); out_mask (shape of the result): the result is zero where out_mask <= 0; bias, then ReLU, before out_mask."""
    x, w, bias, mask, out_mask = map(_i64, (x, w, bias, mask, out_mask))
    xm = x if mask is None else torch.where(mask > 0, x, torch.zeros_like(x))
    y = _conv_raw(xm, w, frames)
    assert_exact_forward(xm, w, bias, frames)
    if bias is not None:
        y = y + bias
    if relu:
        y = y.clamp_min(0)
    if out_mask is not None:
        y = torch.where(out_mask <= 0, torch.zeros_like(y), y)
    return y


def assert_exact_forward(x, w, bias=None, frames=1):
    """sum |term| < 2^24 at every output element of conv3x3(x, w, bias), in int64.  Two cheap per-element upper bounds first -- max |w| times the
    |x| of the element's window summed over all channels, and max |x| times the output channel's sum of |w| -- and the full convolution of the absolute
    values only where neither already stays below 2^24."""
    bmax = int(bias.abs().max()) if bias is not None else 0
    if not x.numel() or not w.numel():
        return
    by_rows = int(w.abs().reshape(w.shape[0], -1).sum(1).max()) * int(x.abs().max()) + bmax
    if by_rows < LIMIT:
        return
    box = _conv_raw(x.abs().sum(3, keepdim=True), torch.ones((1, 1) + tuple(w.shape[2:]), dtype=I64), frames)
    if int(box.max()) * int(w.abs().max()) + bmax < LIMIT:
        return
    ab = _conv_raw(x.abs(), w.abs(), frames)
    _bound('conv3x3', ab + bias.abs() if bias is not None else ab)


def dgrad_weight(w):
    """The weight of the data gradient as a convolution: channels exchanged, every tap mirrored."""
    dims = tuple(range(2, w.dim()))
    return w.transpose(0, 1).flip(dims).contiguous()


def conv3x3_dgrad(gy, w, frames=1, mask=None, out_mask=None):
    """d loss / d x of conv3x3(x, w) given gy = d loss / d y: the convolution of gy with the mirrored, transposed weight.  mask: the forward
    output of the ReLU that follows the layer (gy counts where mask > 0); out_mask: the layer's input when that was a ReLU output."""
    return conv3x3(gy, dgrad_weight(_i64(w)), None, frames, False, mask, out_mask)


def conv3x3_wgrad(gy, x, frames=1, kt=1, mask=None):
    """-> (dw [co,ci,3,3] or [co,ci,3,3,3], db [co]): dw[o,c,(dt,)dy,dx] = sum over images and pixels gy[p,o] x[p + tap,c]."""
    gy, x, mask = map(_i64, (gy, x, mask))
    g = gy if mask is None else torch.where(mask > 0, gy, torch.zeros_like(gy))
    n, h, ww, ci = x.shape
    co = g.shape[3]

    def taps2(gg, xx):
        out = _mm(gg.reshape(-1, co).t().contiguous(), _patches(xx))              # [co, 9*ci], taps in (dy, dx) order
        return out.view(co, 3, 3, xx.shape[3]).permute(0, 3, 1, 2)

    def run(gg, xx):
        if kt == 1:
            return taps2(gg, xx)
        g5, x5 = gg.view(n // frames, frames, h, ww, co), xx.view(n // frames, frames, h, ww, ci)
        out = torch.zeros((co, ci, 3, 3, 3), dtype=I64)
        for dt in range(3):
            lo, hi = max(0, 1 - dt), min(frames, frames + 1 - dt)
            if lo < hi:
                out[:, :, dt] = taps2(g5[:, lo:hi].reshape(-1, h, ww, co), x5[:, lo + dt - 1:hi + dt - 1].reshape(-1, h, ww, ci))
        return out

    dw = run(g, x)
    _bound('conv3x3_wgrad', run(g.abs(), x.abs()))
    db = g.reshape(-1, co).sum(0)
    _bound('conv3x3_wgrad bias', g.abs().reshape(-1, co).sum(0))
    return dw, db


def upconv2x2(x, w, bias=None):
    """2x2 stride-2 transposed convolution: x [n,h,w,ci], w [ci,cu,2,2] -> [n,2h,2w,cu]; y[2y+a, 2x+b, u] = sum_c x[y,x,c] w[c,u,a,b] + bias[u]."""
    x, w, bias = map(_i64, (x, w, bias))
    n, h, ww, ci = x.shape
    cu = w.shape[1]
    y = torch.zeros((n, h, 2, ww, 2, cu), dtype=I64)
    ab = torch.zeros_like(y)
    xm = x.reshape(-1, ci)
    for a in range(2):
        for b in range(2):
            y[:, :, a, :, b] = _mm(xm, w[:, :, a, b]).view(n, h, ww, cu)
            ab[:, :, a, :, b] = _mm(xm.abs(), w[:, :, a, b].abs()).view(n, h, ww, cu)
    if bias is not None:
        y = y + bias
        ab = ab + bias.abs()
    _bound('upconv2x2', ab)
    return y.view(n, 2 * h, 2 * ww, cu)


def upconv2x2_dgrad(gy, w):
    """gy [n,2h,2w,cu], w [ci,cu,2,2] -> [n,h,w,ci]: gx[y,x,c] = sum_{a,b,u} gy[2y+a, 2x+b, u] w[c,u,a,b]."""
    gy, w = map(_i64, (gy, w))
    n, h2, w2, cu = gy.shape
    h, ww, ci = h2 // 2, w2 // 2, w.shape[0]
    g6 = gy.view(n, h, 2, ww, 2, cu)
    gx = torch.zeros((n * h * ww, ci), dtype=I64)
    ab = torch.zeros_like(gx)
    for a in range(2):
        for b in range(2):
            gm = g6[:, :, a, :, b].reshape(-1, cu)
            gx += _mm(gm, w[:, :, a, b].t())
            ab += _mm(gm.abs(), w[:, :, a, b].abs().t())
    _bound('upconv2x2_dgrad', ab)
    return gx.view(n, h, ww, ci)


def upconv2x2_wgrad(gy, x):
    """-> (dw [ci,cu,2,2], db [cu])."""
    gy, x = map(_i64, (gy, x))
    n, h, ww, ci = x.shape
    cu = gy.shape[3]
    g6 = gy.view(n, h, 2, ww, 2, cu)
    xm = x.reshape(-1, ci).t().contiguous()
    dw = torch.zeros((ci, cu, 2, 2), dtype=I64)
    ab = torch.zeros_like(dw)
    for a in range(2):
        for b in range(2):
            gm = g6[:, :, a, :, b].reshape(-1, cu)
            dw[:, :, a, b] = _mm(xm, gm)
            ab[:, :, a, b] = _mm(xm.abs(), gm.abs())
    _bound('upconv2x2_wgrad', ab)
    _bound('upconv2x2_wgrad bias', gy.abs().reshape(-1, cu).sum(0))
    return dw, gy.reshape(-1, cu).sum(0)


# ---- int64 -> the kernels' number formats -------------------------------------------------------------------------------------------------
def exact_f32(t):
    """int64 -> fp32, with the check that the cast lost nothing."""
    f = _i64(t).to(torch.float32)
    assert torch.equal(f.to(I64), t), 'int64 -> fp32 cast is not exact (|value| >= 2^24?)'
    return f


def exact_bf16(t):
    """int64 -> bf16 for OPERANDS: the cast must be exact (at most 8 significant bits)."""
    b = exact_f32(t).to(torch.bfloat16)
    assert torch.equal(b.to(I64), t), 'int64 -> bf16 cast is not exact (more than 8 significant bits?)'
    return b


def rounded_bf16(t):
    """int64 -> fp32 (exact) -> bf16, rounded once to nearest even: what a bf16 epilogue must store."""
    return exact_f32(t).to(torch.bfloat16)


def bf16_rounding_census(t):
    """-> (ties, inexact non-ties) among the elements of an int64 result stored as bf16.  A tie lies exactly between two bf16 neighbours (only
    round-to-nearest-EVEN gets it right); an inexact non-tie tells truncation from rounding."""
    f = exact_f32(t)
    lo = (f.view(torch.int32) & 0xffff)                        # the 16 bits a bf16 store drops
    return int((lo == 0x8000).sum()), int(((lo != 0) & (lo != 0x8000)).sum())


# ---- input families (seeded, deterministic) --------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(int(seed))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=I64)


def _wshape(co, ci, kt):
    return (co, ci, 3, 3, 3) if kt == 3 else (co, ci, 3, 3)


def _sparse_signs(g, shape, per_row):
    """{-1,0,1} weights with at most `per_row` non-zeros per output channel (row = everything behind dim 0)."""
    w = torch.zeros(shape, dtype=I64)
    flat = w.view(shape[0], -1)
    idx = torch.randint(0, flat.shape[1], (shape[0], per_row), generator=g)
    sign = _randint(g, 0, 1, (shape[0], per_row)) * 2 - 1
    flat.scatter_(1, idx, sign)
    return w


def _check_forward(x, w, b, frames):
    assert_exact_forward(x, w, b, frames)                      # raises NotExact when sum |term| >= 2^24 anywhere
    return x, w, b


def dense_small(seed, n, h, w, ci, co, kt=1, frames=1, bf16_out=False):
    """Family 1: activations uniform in {-3..3}, weights in {-1,0,1}, bias in {-4..4} (worst case 27*512*3 + 4 < 2^16).  bf16_out with
    c_in >= 256: the builder asserts that the result holds bf16 ties AND inexact non-ties, so that the store's rounding mode is exercised."""
    g = _gen(seed)
    x = _randint(g, -3, 3, (n, h, w, ci))
    wt = _randint(g, -1, 1, _wshape(co, ci, kt))
    b = _randint(g, -4, 4, (co,))
    if bf16_out and ci >= 256:
        # Zero-mean sums of 9 * 512 terms rarely pass 512, where bf16 neighbours are 4 apart and roundings other than ties begin.  The first 32 output
        # channels get the signs of one pixel's activations (and of its right neighbour's) as their centre (and right) tap: still weights in
        # {-1,0,1}, but coherent sums of about 2 * c_in * 12 / 7 at that pixel -- odd and even integers between 512 and 2047.
        n0, y0, x0 = n - 1, h // 2, max(0, w // 2 - 1)
        taps = (1,) if wt.dim() == 5 else ()                   # the centre frame tap of a 3x3x3 weight
        for dx in range(min(2, w - x0)):
            s = x[n0, y0, x0 + dx].sign()
            keep = s != 0
            wt[(slice(0, min(32, co)), keep) + taps + (1, 1 + dx)] = s[keep]
    _check_forward(x, wt, b, frames)
    if bf16_out and ci >= 256:
        ties, inexact = bf16_rounding_census(conv3x3(x, wt, b, frames))
        assert ties > 0 and inexact > 0, 'dense_small: no bf16 tie / no inexact non-tie in the result (%d, %d)' % (ties, inexact)
    return x, wt, b


def position_hash(n, h, w, c):
    """[n,h,w,c] int64 in {-3..3}: a small integer hash of the element's coordinates (img, y, x, channel)."""
    i = torch.arange(n, dtype=I64).view(n, 1, 1, 1)
    y = torch.arange(h, dtype=I64).view(1, h, 1, 1)
    x = torch.arange(w, dtype=I64).view(1, 1, w, 1)
    ch = torch.arange(c, dtype=I64).view(1, 1, 1, c)
    v = (i * 7919 + y * 104729 + x * 1299709 + ch * 15485863 + 12345) % 2147483647
    v = (v * 48271) % 2147483647                               # one Lehmer step: neighbours in any direction get unrelated values
    return (v >> 7) % 7 - 3


def position_code(seed, n, h, w, ci, co, kt=1, frames=1):
    """Family 2: activations = position_hash, weights one-hot per output channel -- channel o reads input channel src_c[o] through tap
    src_tap[o] (both vary with o), so every output element names the one input element it read.  -> (x, w, None, (src_tap, src_c))."""
    g = _gen(seed)
    x = position_hash(n, h, w, ci)
    taps = 9 * kt
    src_tap = (torch.arange(co, dtype=I64) * 5 + 1 + int(seed)) % taps
    src_c = torch.randperm(max(ci, co), generator=g)[:co] % ci
    wt = torch.zeros((co, ci, taps), dtype=I64)
    wt[torch.arange(co), src_c, src_tap] = 1
    wt = wt.view(_wshape(co, ci, kt))
    _check_forward(x, wt, None, frames)
    return x, wt, None, (src_tap, src_c)


def explain_position(x, frames, kt, code, where, got):
    """For a mismatch of a position-code case at where = (img, y, x, o): the element that should have been read, and -- if one exists -- an
    element of the same input channel in the 5x5 neighbourhood of the current, adjacent frame or image that holds the value the kernel gave."""
    src_tap, src_c = code
    img, y, xx, o = where
    n, h, w, _ = x.shape
    tap, c = int(src_tap[o]), int(src_c[o])
    dt, dy, dx = (tap // 9 - 1 if kt == 3 else 0), tap % 9 // 3 - 1, tap % 3 - 1
    msg = 'output (img %d, y %d, x %d, ch %d) reads input (img %d, y %d, x %d, ch %d)' % (img, y, xx, o, img + dt, y + dy, xx + dx, c)
    t = img % frames
    if not (0 <= t + dt < frames and 0 <= y + dy < h and 0 <= xx + dx < w):
        msg += ' -- outside the image / sample: zero'
    if got != got or got != int(got):
        return msg + '; the kernel gave %r, which no input element holds' % (got,)
    for di in (0, -1, 1):
        for ey in range(-2, 3):
            for ex in range(-2, 3):
                if (di, ey, ex) == (dt, dy, dx):
                    continue
                ii, yy, xs = img + di, y + ey, xx + ex
                if 0 <= ii < n and 0 <= yy < h and 0 <= xs < w and int(x[ii, yy, xs, c]) == int(got) and int(got) != 0:
                    return msg + '; the kernel gave %d = input (img %d, y %d, x %d, ch %d)' % (int(got), ii, yy, xs, c)
    return msg + '; the kernel gave %d, found nowhere in the 5x5 neighbourhood of the adjacent frames / images of that channel' % int(got)


def lo_plane_bits(t):
    """How many elements of an int64 operand have a non-zero fp16 lo half after the fp32x3 tensor scale (a power of two that puts the
    absolute maximum into [2^13, 2^14)): hi = fp16(s t), lo = fp16(s t - hi).  Also asserts hi + lo == s t (the split itself is exact)."""
    f = exact_f32(t)
    amax = float(f.abs().max())
    if amax == 0.0:
        return 0
    import math
    s = 2.0 ** (14 - math.frexp(amax)[1])
    hi = (f * s).to(torch.float16)
    lo = (f * s - hi.float()).to(torch.float16)
    assert torch.equal(hi.float() + lo.float(), f * s), 'hi + lo does not carry the operand exactly'
    return int((lo != 0).sum())


def lo_activations(seed, n, h, w, ci, co, kt=1, frames=1, bits=20, per_row=8):
    """Family 3a: activations = integers of up to `bits` significant bits (hi and lo halves both non-zero after scaling), weights in {-1,0,1}
    with at most `per_row` non-zeros per output channel: 8 * 2^20 = 2^23 < 2^24.  w_lo is zero, x_lo is not: only w_hi*x_lo carries it."""
    g = _gen(seed)
    top = (1 << bits) - 1
    x = _randint(g, -top, top, (n, h, w, ci))
    wt = _sparse_signs(g, _wshape(co, ci, kt), per_row)
    _check_forward(x, wt, None, frames)
    assert lo_plane_bits(x) > 0, 'lo_activations: every lo half is zero'
    return x, wt, None


def lo_weights(seed, n, h, w, ci, co, kt=1, frames=1, per_row=6):
    """Family 3b, the mirror image: weights = 18- to 20-bit integers at `per_row` places of each output channel (zero elsewhere; the row scale is a
    power of two of the row's maximum), activations sparse in {-1,0,1}.  Only w_lo*x_hi carries the lo plane.  per_row * 2^20 < 2^24."""
    g = _gen(seed)
    x = _randint(g, -1, 1, (n, h, w, ci)) * _randint(g, 0, 1, (n, h, w, ci))      # two thirds zeros
    shape = _wshape(co, ci, kt)
    wt = torch.zeros(shape, dtype=I64)
    flat = wt.view(co, -1)
    idx = torch.randint(0, flat.shape[1], (co, per_row), generator=g)
    mag = _randint(g, 1 << 17, (1 << 20) - 1, (co, per_row)) | 1                 # odd: the low bit is in use
    flat.scatter_(1, idx, mag * (_randint(g, 0, 1, (co, per_row)) * 2 - 1))
    _check_forward(x, wt, None, frames)
    rows_lo = sum(lo_plane_bits(wt[o]) for o in range(0, co, max(1, co // 8)))
    assert rows_lo > 0, 'lo_weights: every lo half is zero'
    return x, wt, None


def bf16_mantissa(seed, n, h, w, ci, co, kt=1, frames=1, per_row=16):
    """Family 4: activations with all 8 significant bits of bf16 in use (|x| <= 255, odd values included), weights sparse in {-1,0,1}."""
    g = _gen(seed)
    x = _randint(g, -255, 255, (n, h, w, ci))
    x[..., 0] |= 1                                                              # odd values in every pixel
    wt = _sparse_signs(g, _wshape(co, ci, kt), per_row)
    b = _randint(g, -4, 4, (co,))
    _check_forward(x, wt, b, frames)
    exact_bf16(x)
    return x, wt, b


def small_grad(seed, shape, lo=-3, hi=3):
    """An incoming gradient / second operand of the gradient kernels: uniform integers in {lo..hi}."""
    return _randint(_gen(seed), lo, hi, shape)


def relu_like_mask(seed, shape):
    """A mask map as a ReLU output is: about half zeros, the rest positive; a few negatives to tell `<= 0` from `== 0` and `< 0`."""
    g = _gen(seed)
    m = _randint(g, -1, 3, shape)
    return torch.where(m == 2, torch.zeros_like(m), m)                            # values {-1, 0, 0, 1, 3}: zeros, negatives and positives all present
