"""The 3x3 / 3x3x3 / 2x2 convolution stacks (csrc/conv.hip, conv_deep.hip, conv_split.hip, head_conv.hip, upconv_bf16.hip) held to EXACT integer
results at every element.

On small-integer operands every product and partial sum is an integer below 2^24: exact as a bf16 product, as an fp16 hi / lo product of the
power-of-two scaled fp32x3 operands and as an fp32 FMA, so summation order, atomics, partial slots and the MFMA layout cannot change a bit.  The
kernel must equal the int64 reference of tests/conv_exact_reference.py bit for bit (torch.equal on the whole tensor; bf16 outputs equal the reference
rounded once to nearest even).  There is no tolerance anywhere in this file and no element is excluded: a lost halo channel, a stale element of a ragged
strip, a truncating store, a frame leaking across a sample boundary, a wrong mask predicate each change at least one element by at least one unit.

Input families (conv_exact_reference.py): 1 dense small integers (with bf16 ties at c_in >= 256), 2 position code (one-hot weights: every output
element names the input element it read; a mismatch prints where the value came from), 3a / 3b fp32x3 lo planes (20-bit activations / weights: the
w_hi*x_lo and w_lo*x_hi products carry bits the hi*hi product does not), 4 bf16 mantissa (all 8 significant bits in use).

Which kernel variant a shape reaches
------------------------------------
bf16 resident kernels (conv.hip, conv3x3_bf16_any): c_in 32 -> c_out 32 / 64 / 128 at kt = 1 are (1,32,2,1) / (2,32,2,2) / (4,32,2,2); every
c_in = 32, kt = 3 layer is the 27-tap (1,32,1,1) kernel, swizzled or (PCACC_CONV_SWZ_OFF) padded; c_in 64 -> 32 is (1,64,1,1), 64 -> 64 / 128 is
(2,64,2,1).  Unreachable at any shape: (2,32,2,1) and (1,64,2,1) -- the `alone` test (LDS > 80 KB) is decided by (c_in, c_out group, kt) alone, and
those two combinations never fall on that side of it.  c_in = 64 with kt = 3 does not fit the resident LDS budget and runs the generic kernel.
bf16 generic kernels (conv3x3_mfma_kernel<CT, CS>): CS = 32 / 64 / 128 from c_in 96 / 192 / 128, CT = 1 / 2 / 4 from c_out 32 / 64 / 128; reached at
kt = 1 where the strip planner refuses the layer (c_in = 96, c_out = 32) and at kt = 3 otherwise -- GENERIC below, nine cases.

Strip kernels and fp32x3 planners: found with the planners themselves, swept over every n <= 3, h, w <= 80, channels <= 512 in steps of 32.  The
table is (n, h, w, c_in, c_out) -> the plan the launcher prints under PCACC_CONV_PLAN; the tests assert each line and that together they are the
whole reachable set.

    conv_deep.hip strip kernel (cs, ng, mt)                      fp32x3 tiled kernel (cs, nw, ngw, mt), PCACC_CONV_RES=0
    (2,  7,  5, 128,  64)  (64,1,1)  one ragged strip            (2,  7,  5,  32,  32)  (32,1,1,1)   (1, 19, 37,  32,  64)  (32,1,1,1) bands of 19
    (1, 19, 37, 128, 192)  (64,1,1)  rows 5 of 19                (1, 18, 18,  64,  64)  (64,1,1,1)   (1, 33, 70,  32,  32)  (32,1,1,1) bands of 24
    (1, 33, 70, 128,  64)  (64,1,1)  rows 3 of 33                (1,  1, 40,  64,  32)  (64,1,1,1)   (1,  5, 72,  64,  64)  (64,1,1,1) bands of 24
    (1,  5, 72, 192, 128)  (64,1,1)  rows 3 of 5                 (1,  7,  5, 128, 256)  (64,1,1,1)   (2,  9, 33,  96,  64)  (32,1,1,1)
    (1, 18, 18, 256, 128)  (64,2,1)                              (3, 21, 52,  32, 480)  (32,1,1,2)   (3, 21, 52,  64, 480)  (64,1,1,2)
    (1,  1, 40, 128, 128)  (64,2,1)  single row                  (3, 31, 74,  32, 480)  (32,1,1,3)
    (1,  7,  5, 512, 512)  (64,2,1)  bf16 ties                   (2, 37, 52,  32, 448)  (32,2,1,1)   (2, 37, 52,  64, 448)  (64,2,1,1)
    (3, 31, 65, 128, 512)  (64,1,2)                              (3, 65, 77,  32, 320)  (32,2,1,2)
    (3, 31, 70, 128, 512)  (64,2,2)                              (3, 21, 52,  32, 512)  (32,2,2,1)   (3, 21, 52,  64, 512)  (64,2,2,1)
    (3, 64, 70, 128, 512)  (64,2,3)                              (3, 37, 75,  32, 512)  (32,2,2,2)   (3, 36, 75,  64, 512)  (64,2,2,2)
    (2,  9,  1, 128, 128)  (64,2,1)  one column                  (2,  9,  1,  64,  32)  (64,1,1,1) one column

    fp32x3 resident kernel (cs, nw, mt, restage), PCACC_CONV_RES=2: restage = more than one (frame tap, channel slice) per tile
    (2,  7,  5, 32, 32) (32,1,1,-)   (1, 19, 37, 32, 64) (32,2,1,-)   (1,  1, 40, 64, 32) (64,1,1,-)   (1, 25, 57, 32, 32) (32,1,2,-)
    (1, 79,  6, 64, 32) (32,1,1,R)   (1, 18, 18, 64, 64) (32,2,1,R)   (1, 25, 57, 64, 32) (32,1,2,R)   kt = 3 of (1, 1, 40, 64, 32): (64,1,1,R)

Instantiated but unreachable in that range (n <= 3, h, w <= 80, channels <= 512), hence not run here:
  * strip kernels with cs = 32, all five (ng, mt): a 64-channel slice fits the staging budget for every patch of at most 82 x 82 pixels;
  * fp32x3 tiled (64,2,1,2) and (64,1,1,3): with 64-channel slices the planner's cost model prefers (64,2,2,mt) resp. a smaller mt wherever those
    would fit (they appear on wider maps only).
The multi-tile variants (mt >= 2, nw = 2) need more than 256 workgroups before the cost model picks them, which is why their shapes are the largest
in this file (the int64 reference of the largest takes about two seconds).

Order-dependent contracts: none was found.  Every case below is exact; the cap on excluded elements is zero."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
from pcaccumulation_amd import native, ops

gpu = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _dev():
    return torch.device('cuda:0')


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
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


def _bf(t):
    return R.exact_bf16(t).to(_dev())


def _f(t):
    return R.exact_f32(t).to(_dev())


def _plan_lines(capfd, prefix):
    err = capfd.readouterr().err
    return [ln for ln in err.splitlines() if ln.startswith(prefix)]


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


# ---- shared references: built once per (family, shape), never written to ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(name, seed, n, h, w, ci, co, kt, frames, bf16_out=False):
    if name == 'dense':
        x, wt, b = R.dense_small(seed, n, h, w, ci, co, kt, frames, bf16_out=bf16_out)
        code = None
    elif name == 'position':
        x, wt, b, code = R.position_code(seed, n, h, w, ci, co, kt, frames)
    elif name == 'lo_x':
        x, wt, b = R.lo_activations(seed, n, h, w, ci, co, kt, frames)
        code = None
    elif name == 'lo_w':
        x, wt, b = R.lo_weights(seed, n, h, w, ci, co, kt, frames)
        code = None
    else:
        x, wt, b = R.bf16_mantissa(seed, n, h, w, ci, co, kt, frames)
        code = None
    return x, wt, b, code


@functools.lru_cache(maxsize=None)
def _forward_ref(name, seed, n, h, w, ci, co, kt, frames, bias, relu, bf16_out=False):
    x, wt, b, _ = _family(name, seed, n, h, w, ci, co, kt, frames, bf16_out)
    return R.conv3x3(x, wt, b if bias else None, frames, relu)


def _explainer(x, frames, kt, code):
    return None if code is None else (lambda where, got: R.explain_position(x, frames, kt, code, where, got))


# =========================================================================================================================================
# CPU self-checks: the reference against the library in float64, the families against their own conditions
# =========================================================================================================================================
def _lib_conv(x, wt, b, frames):
    xd, wd = x.double(), wt.double()
    bd = b.double() if b is not None else None
    if wt.dim() == 5:
        n, h, w, ci = x.shape
        x5 = xd.view(n // frames, frames, h, w, ci).permute(0, 4, 1, 2, 3)
        return F.conv3d(x5, wd, bd, padding=1).permute(0, 2, 3, 4, 1).reshape(n, h, w, -1)
    return F.conv2d(xd.permute(0, 3, 1, 2), wd, bd, padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize('n,frames,h,w,ci,co,kt', [(2, 1, 5, 7, 8, 6, 1), (1, 1, 1, 1, 4, 4, 1), (6, 3, 4, 5, 4, 8, 3), (4, 2, 3, 3, 8, 4, 3),
                                                   (2, 1, 3, 9, 4, 4, 3)])
def test_reference_matches_the_library_in_float64(n, frames, h, w, ci, co, kt):
    """conv3x3 and its three gradients == F.conv2d / F.conv3d and autograd in float64 on the same integers, masks and frame / sample boundaries
    included (frames = 1 with kt = 3: every frame is a sample of its own)."""
    x, wt, b = R.dense_small(3, n, h, w, ci, co, kt, frames)
    mask, omask = R.relu_like_mask(4, x.shape), R.relu_like_mask(5, (n, h, w, co))
    gy = R.small_grad(6, (n, h, w, co))
    assert mask.numel() < 100 or {-1, 0, 1, 3} <= set(mask.unique().tolist())
    xd = x.double().requires_grad_(True)
    wd, bd = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    y = _lib_conv(xd, wd, bd, frames)
    assert torch.equal(R.conv3x3(x, wt, b, frames).double(), y.detach())
    assert torch.equal(R.conv3x3(x, wt, None, frames, relu=True).double(), torch.relu(_lib_conv(x, wt, None, frames)))
    assert torch.equal(R.conv3x3(x, wt, b, frames, mask=mask).double(), _lib_conv(x * (mask > 0), wt, b, frames))
    assert torch.equal(R.conv3x3(x, wt, None, frames, out_mask=omask).double(), _lib_conv(x, wt, None, frames) * (omask > 0))
    # gradients through a ReLU: the mask is the forward output
    yr = torch.relu(y)
    yr.backward(gy.double())
    y_int = R.conv3x3(x, wt, b, frames, relu=True)
    assert torch.equal(R.conv3x3_dgrad(gy, wt, frames, mask=y_int).double(), xd.grad)
    dw, db = R.conv3x3_wgrad(gy, x, frames, kt, mask=y_int)
    assert torch.equal(dw.double(), wd.grad) and torch.equal(db.double(), bd.grad)
    assert torch.equal(R.conv3x3_dgrad(gy, wt, frames, out_mask=mask).double(), torch.where(mask <= 0, 0.0, R.conv3x3_dgrad(gy, wt, frames).double()))


def test_reference_frames_do_not_cross_samples():
    """A 3x3x3 layer on two samples == the same layer on each sample alone: nothing leaks across the boundary, first and last frames see zeros."""
    x, wt, b = R.dense_small(9, 6, 3, 4, 4, 4, 3, 3)
    both = R.conv3x3(x, wt, b, 3)
    assert torch.equal(both[:3], R.conv3x3(x[:3], wt, b, 3)) and torch.equal(both[3:], R.conv3x3(x[3:], wt, b, 3))
    x2 = x.clone()
    x2[2] += 1                                                 # the last frame of sample 0 must not reach sample 1
    assert torch.equal(R.conv3x3(x2, wt, b, 3)[3:], both[3:])


@pytest.mark.parametrize('n,h,w,ci,cu', [(2, 3, 5, 8, 4), (1, 1, 1, 4, 4)])
def test_upconv_reference_matches_the_library_in_float64(n, h, w, ci, cu):
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (n, h, w, ci), generator=g)
    wt = torch.randint(-2, 3, (ci, cu, 2, 2), generator=g)
    b = torch.randint(-4, 5, (cu,), generator=g)
    gy = torch.randint(-3, 4, (n, 2 * h, 2 * w, cu), generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wt, b))
    y = F.conv_transpose2d(xd.permute(0, 3, 1, 2), wd, bd, stride=2).permute(0, 2, 3, 1)
    y.backward(gy.double())
    assert torch.equal(R.upconv2x2(x, wt, b).double(), y.detach())
    assert torch.equal(R.upconv2x2_dgrad(gy, wt).double(), xd.grad)
    dw, db = R.upconv2x2_wgrad(gy, x)
    assert torch.equal(dw.double(), wd.grad) and torch.equal(db.double(), bd.grad)


def test_families_hold_their_own_conditions():
    """Every family passes its 2^24 assertion at the largest channel counts it is used with; the tie and lo-plane presence assertions hold; a family
    that is NOT exact is refused."""
    for shape in ((1, 7, 5, 512, 512), (1, 18, 18, 256, 128), (2, 18, 18, 256, 128)):                    # the bf16 cases with c_in >= 256
        ties, inexact = R.bf16_rounding_census(R.conv3x3(*R.dense_small(sum(shape), *shape, bf16_out=True)))      # asserted inside the builder too
        assert ties > 0 and inexact > 0, (shape, ties, inexact)
    R.dense_small(2, 6, 5, 9, 32, 128, 3, 3)
    for build in (R.lo_activations, R.lo_weights):
        for ci, co, kt, frames in ((32, 32, 1, 1), (128, 256, 1, 1), (64, 32, 3, 2)):
            x, wt, _ = build(5, 2 * frames, 7, 5, ci, co, kt, frames)
            assert R.lo_plane_bits(x if build is R.lo_activations else wt[0]) > 0
    x, wt, b = R.bf16_mantissa(7, 2, 7, 5, 256, 64)
    assert int(x.abs().max()) == 255 and bool((x % 2 != 0).any())
    _, wt, _, (tap, ch) = R.position_code(3, 2, 5, 6, 32, 64)
    assert bool((wt.view(64, -1).sum(1) == 1).all()) and int(wt.abs().sum()) == 64 and len(set(tap.tolist())) == 9 and len(set(ch.tolist())) == 32      # one-hot rows; every tap and channel in use
    assert set(R.position_hash(2, 9, 9, 32).unique().tolist()) == set(range(-3, 4))
    with pytest.raises(R.NotExact):
        R.conv3x3(torch.full((1, 3, 3, 32), 1 << 20, dtype=torch.int64), torch.ones((32, 32, 3, 3), dtype=torch.int64))
    with pytest.raises(AssertionError):
        R.exact_f32(torch.tensor([(1 << 24) + 1]))
    assert R.rounded_bf16(torch.tensor([257, 259, 261, 258])).tolist() == [256.0, 260.0, 260.0, 258.0]      # ties to even; 258 is exact


def test_position_code_names_the_element_that_was_read():
    x, wt, _, code = R.position_code(1, 4, 6, 7, 32, 32, 3, 2)
    y = R.conv3x3(x, wt, None, 2)
    for img, yy, xx, o in ((2, 3, 3, 5), (0, 0, 0, 7), (3, 5, 6, 30), (1, 2, 4, 11)):
        tap, ch = int(code[0][o]), int(code[1][o])
        dt, dy, dx = tap // 9 - 1, tap % 9 // 3 - 1, tap % 3 - 1
        inside = 0 <= img % 2 + dt < 2 and 0 <= yy + dy < 6 and 0 <= xx + dx < 7
        assert int(y[img, yy, xx, o]) == (int(x[img + dt, yy + dy, xx + dx, ch]) if inside else 0)
    assert 'reads input' in R.explain_position(x, 2, 3, code, (2, 3, 3, 5), 2.0)


# =========================================================================================================================================
# bf16: csrc/conv.hip resident and generic kernels
# =========================================================================================================================================
HW = [(1, 1), (7, 31), (8, 32), (9, 33), (17, 65)]              # straddle the 8 x 32 tile
RESIDENT = [(32, 32, 1), (32, 64, 1), (32, 128, 1), (64, 32, 1), (64, 64, 1), (64, 128, 1), (32, 32, 3), (32, 64, 3), (32, 128, 3)]


def _bf16_forward_cases(n, frames, h, w, ci, co, kt, seed, outmask=True):
    """The forward checks every bf16 kernel gets: dense with and without bias / ReLU, position code, bf16 mantissa, out_mask."""
    for fam, bias, relu in (('dense', True, True), ('dense', False, False), ('position', False, False), ('mantissa', True, False)):
        x, wt, b, code = _family(fam, seed, n, h, w, ci, co, kt, frames, fam == 'dense')
        wp = native.conv3x3_prepare_weights(_f(wt))
        y = native.conv3x3(_bf(x), wp, _f(b) if bias else None, frames, relu)
        _same(y, _forward_ref(fam, seed, n, h, w, ci, co, kt, frames, bias, relu, fam == 'dense'), BF16,
              '%s bias=%s relu=%s frames=%d' % (fam, bias, relu, frames), _explainer(x, frames, kt, code))
    if outmask:
        x, wt, b, _ = _family('dense', seed, n, h, w, ci, co, kt, frames, True)
        om = R.relu_like_mask(seed + 1, (n, h, w, co))
        assert native.conv3x3_outmask_supported(h, w, ci, co, kt)
        y = native.conv3x3(_bf(x), native.conv3x3_prepare_weights(_f(wt)), None, frames, False, out_mask=_bf(om))
        _same(y, R.conv3x3(x, wt, None, frames, out_mask=om), BF16, 'out_mask frames=%d' % frames)


@gpu
@pytest.mark.parametrize('h,w', HW)
@pytest.mark.parametrize('ci,co,kt,swz_off', [c + (False,) for c in RESIDENT] + [c + (True,) for c in RESIDENT if c[2] == 3])
def test_bf16_resident_forward(ci, co, kt, swz_off, h, w, switches):
    """Every (ctr, alone) branch of conv3x3_bf16_any, the 27-tap layer swizzled and padded; kt = 3 on two samples of 1, 2 and 3 frames."""
    if swz_off:
        switches(PCACC_CONV_SWZ_OFF='1')
    for frames in ((1, 2, 3) if kt == 3 and h * w < 1000 else (2,) if kt == 3 else (1,)):
        _bf16_forward_cases(2 * frames, frames, h, w, ci, co, kt, seed=ci + co + kt + h)


GENERIC = [(96, 32, 1), (96, 64, 1), (96, 128, 1), (192, 32, 1), (192, 64, 3), (192, 128, 3), (128, 32, 1), (128, 64, 3), (128, 128, 3)]


@gpu
@pytest.mark.parametrize('ci,co,kt', GENERIC + [(64, 64, 3)])
def test_bf16_generic_forward(ci, co, kt):
    """All nine (ct, cs_sel) of the generic kernel: layers the strip planner refuses (asserted), or 3x3x3 layers."""
    h, w = 9, 33
    frames = 2 if kt == 3 else 1
    if kt == 1:
        assert not native.conv3x3_deep_supported(h, w, ci, co)
    elif ci >= 128:
        assert native.conv3x3_deep_supported(h, w, ci, co)        # the strip kernel would take it as a 3x3 layer: kt = 3 keeps it here
    _bf16_forward_cases(2 * frames, frames, h, w, ci, co, kt, seed=ci + co)


# ---- bf16 weight gradient (conv.hip) -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('h,w', [(1, 1), (9, 33), (17, 65)])
@pytest.mark.parametrize('ci,co,kt', [(32, 32, 1), (64, 32, 1), (32, 64, 1), (64, 64, 1), (32, 32, 3), (64, 64, 3)])
def test_bf16_wgrad(ci, co, kt, h, w):
    for frames in ((1, 2, 3) if kt == 3 else (1,)):
        n = 2 * frames
        x = R.small_grad(ci + h, (n, h, w, ci))
        gy = R.small_grad(co + w, (n, h, w, co))
        dw_ref, db_ref = R.conv3x3_wgrad(gy, x, frames, kt)
        if kt == 1:
            dw, db = native.conv3x3_wgrad(_bf(gy), _bf(x))
            dw = dw.view(co, 3, 3, ci).permute(0, 3, 1, 2)
        else:
            parts = [native.conv3x3_wgrad(_bf(gy), _bf(x), frames, dt) for dt in (-1, 0, 1)]      # the three launches of a kt = 3 layer
            dw = torch.stack([p[0].view(co, 3, 3, ci) for p in parts], 1).permute(0, 4, 1, 2, 3)
            db = parts[1][1]
        _same(dw, dw_ref, F32, 'dW frames=%d' % frames)
        _same(db, db_ref, F32, 'db frames=%d' % frames)


# =========================================================================================================================================
# bf16: csrc/conv_deep.hip strip kernels
# =========================================================================================================================================
STRIP = {   # (n, h, w, c_in, c_out) -> (cs, ng, mt): the table of the module docstring
    (2, 7, 5, 128, 64): (64, 1, 1), (2, 9, 1, 128, 128): (64, 2, 1), (1, 19, 37, 128, 192): (64, 1, 1), (1, 33, 70, 128, 64): (64, 1, 1), (1, 5, 72, 192, 128): (64, 1, 1),
    (1, 18, 18, 256, 128): (64, 2, 1), (1, 1, 40, 128, 128): (64, 2, 1), (1, 7, 5, 512, 512): (64, 2, 1),
    (3, 31, 65, 128, 512): (64, 1, 2), (3, 31, 70, 128, 512): (64, 2, 2), (3, 64, 70, 128, 512): (64, 2, 3)}
STRIP_REACHABLE = {(64, 1, 1), (64, 1, 2), (64, 2, 1), (64, 2, 2), (64, 2, 3)}


def _strip_plan(capfd, shape):
    lines = _plan_lines(capfd, 'conv plan %dx%d %d->%d n=%d:' % (shape[1], shape[2], shape[3], shape[4], shape[0]))
    assert lines, 'no plan line for %s' % (shape,)
    m = re.search(r'cs=(\d+) ng=(\d+) mt=(\d+)', lines[-1])
    return tuple(int(v) for v in m.groups())


@gpu
@pytest.mark.parametrize('shape', sorted(STRIP))
def test_bf16_strip_forward_and_input_mask(shape, switches, capfd):
    n, h, w, ci, co = shape
    assert native.conv3x3_deep_supported(h, w, ci, co) and not native.conv3x3_outmask_supported(h, w, ci, co)
    switches(PCACC_CONV_PLAN='1')
    capfd.readouterr()
    big = n * h * w > 4000
    for fam, bias, relu in (('dense', True, True),) if big else (('dense', True, True), ('dense', False, False), ('position', False, False),
                                                                 ('mantissa', True, False)):
        x, wt, b, code = _family(fam, ci + h, n, h, w, ci, co, 1, 1, fam == 'dense')
        y = native.conv3x3(_bf(x), native.conv3x3_prepare_weights(_f(wt)), _f(b) if bias else None, 1, relu)
        _same(y, _forward_ref(fam, ci + h, n, h, w, ci, co, 1, 1, bias, relu, fam == 'dense'), BF16, '%s bias=%s relu=%s' % (fam, bias, relu),
              _explainer(x, 1, 1, code))
    assert _strip_plan(capfd, shape) == STRIP[shape]
    # the deep input mask: elements read as zero where mask <= 0 (the ReLU backward fused into the staging)
    x, wt, b, _ = _family('dense', ci + h, n, h, w, ci, co, 1, 1, True)
    m = R.relu_like_mask(h + w, x.shape)
    y = native.conv3x3(_bf(x), native.conv3x3_prepare_weights(_f(wt)), _f(b), 1, False, mask=_bf(m))
    _same(y, R.conv3x3(x, wt, b, 1, False, mask=m), BF16, 'input mask')


@gpu
def test_strip_shapes_reach_every_reachable_variant(switches, capfd):
    """The shapes of STRIP together reach every (cs, ng, mt) any shape with n <= 3, h, w <= 80, channels <= 512 reaches (module docstring)."""
    switches(PCACC_CONV_PLAN='1')
    capfd.readouterr()
    seen = set()
    for shape in sorted(STRIP):
        n, h, w, ci, co = shape
        native.conv3x3(torch.zeros((n, h, w, ci), dtype=BF16, device=_dev()), torch.zeros((9, co, ci), dtype=BF16, device=_dev()), None, 1, False)
        torch.cuda.synchronize()
        seen.add(_strip_plan(capfd, shape))
    assert seen == STRIP_REACHABLE


WGRAD_DEEP = [(2, 7, 5, 128, 128), (1, 19, 37, 64, 192), (2, 18, 18, 256, 128), (1, 33, 70, 128, 64), (1, 1, 40, 128, 128), (1, 5, 301, 64, 128),
              (1, 7, 5, 512, 512)]


@gpu
@pytest.mark.parametrize('n,h,w,ci,co', WGRAD_DEEP)
def test_bf16_wgrad_deep(n, h, w, ci, co):
    """pcacc_conv3x3_wgrad_deep_bf16 with and without the ReLU mask; (1, 5, 301) is wider than one strip: column segments with their own halos."""
    assert native.conv3x3_wgrad_deep_supported(h, w, ci, co)
    x = R.small_grad(ci + h, (n, h, w, ci))
    gy = R.small_grad(co + w, (n, h, w, co))
    mask = R.relu_like_mask(h * w, gy.shape)
    for m in (None, mask):
        dw, db = native.conv3x3_wgrad_deep(_bf(gy), _bf(x), mask=_bf(m) if m is not None else None)
        dw_ref, db_ref = R.conv3x3_wgrad(gy, x, 1, 1, mask=m)
        _same(dw.view(co, 3, 3, ci).permute(0, 3, 1, 2), dw_ref, F32, 'dW mask=%s' % (m is not None))
        _same(db, db_ref, F32, 'db mask=%s' % (m is not None))


# ---- the full autograd path of ops.conv3x3_rows (bf16) ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n,frames,h,w,ci,co,kt', [(2, 1, 9, 33, 32, 64, 1), (2, 1, 17, 65, 64, 32, 1), (6, 3, 7, 31, 32, 32, 3), (4, 2, 9, 33, 32, 64, 3),
                                                   (2, 1, 18, 18, 256, 128, 1), (1, 1, 19, 37, 128, 256, 1), (2, 1, 7, 5, 128, 128, 1)])
def test_bf16_autograd_path(n, frames, h, w, ci, co, kt):
    """dX, dW and db of ops.conv3x3_rows (conv + bias + ReLU) with the ReLU mask taken from the REFERENCE: y > 0 is exact here."""
    if ci > 64:                                                # the layer must stay on the project's kernels: a library gradient rounds dW to bf16
        assert native.conv3x3_deep_supported(h, w, ci, co) and native.conv3x3_deep_supported(h, w, co, ci) and native.conv3x3_wgrad_deep_supported(h, w, ci, co)
    else:
        assert native.conv3x3_wgrad_supported(ci, co)
    x, wt, b, _ = _family('dense', ci + co + kt, n, h, w, ci, co, kt, frames, True)
    gy = R.small_grad(co + h, (n, h, w, co))
    xg = _bf(x).requires_grad_(True)
    wg, bg = _f(wt).requires_grad_(True), _f(b).requires_grad_(True)
    y = ops.conv3x3_rows(xg, wg, bg, frames, True)
    y_ref = R.conv3x3(x, wt, b, frames, relu=True)
    _same(y, y_ref, BF16, 'y')
    y.backward(_bf(gy))
    _same(xg.grad, R.conv3x3_dgrad(gy, wt, frames, mask=y_ref), BF16, 'dX')
    dw_ref, db_ref = R.conv3x3_wgrad(gy, x, frames, kt, mask=y_ref)
    _same(wg.grad, dw_ref, F32, 'dW')
    _same(bg.grad, db_ref, F32, 'db')


# =========================================================================================================================================
# fp32x3: csrc/conv_split.hip
# =========================================================================================================================================
SPLIT_TILED = {   # (n, h, w, c_in, c_out) -> (cs, nw, ngw, mt) under PCACC_CONV_RES=0
    (2, 7, 5, 32, 32): (32, 1, 1, 1), (1, 19, 37, 32, 64): (32, 1, 1, 1), (1, 33, 70, 32, 32): (32, 1, 1, 1), (2, 9, 33, 96, 64): (32, 1, 1, 1),
    (1, 18, 18, 64, 64): (64, 1, 1, 1), (1, 1, 40, 64, 32): (64, 1, 1, 1), (2, 9, 1, 64, 32): (64, 1, 1, 1), (1, 5, 72, 64, 64): (64, 1, 1, 1), (1, 7, 5, 128, 256): (64, 1, 1, 1),
    (3, 21, 52, 32, 480): (32, 1, 1, 2), (3, 21, 52, 64, 480): (64, 1, 1, 2), (3, 31, 74, 32, 480): (32, 1, 1, 3),
    (2, 37, 52, 32, 448): (32, 2, 1, 1), (2, 37, 52, 64, 448): (64, 2, 1, 1), (3, 65, 77, 32, 320): (32, 2, 1, 2),
    (3, 21, 52, 32, 512): (32, 2, 2, 1), (3, 21, 52, 64, 512): (64, 2, 2, 1), (3, 37, 75, 32, 512): (32, 2, 2, 2), (3, 36, 75, 64, 512): (64, 2, 2, 2)}
SPLIT_TILED_REACHABLE = {(32, 1, 1, 1), (32, 1, 1, 2), (32, 1, 1, 3), (32, 2, 1, 1), (32, 2, 1, 2), (32, 2, 2, 1), (32, 2, 2, 2),
                         (64, 1, 1, 1), (64, 1, 1, 2), (64, 2, 1, 1), (64, 2, 2, 1), (64, 2, 2, 2)}
SPLIT_RESIDENT = {   # (n, h, w, c_in, c_out, kt) -> (cs, nw, mt, restage) under PCACC_CONV_RES=2
    (2, 7, 5, 32, 32, 1): (32, 1, 1, False), (1, 19, 37, 32, 64, 1): (32, 2, 1, False), (1, 1, 40, 64, 32, 1): (64, 1, 1, False),
    (1, 25, 57, 32, 32, 1): (32, 1, 2, False), (1, 79, 6, 64, 32, 1): (32, 1, 1, True), (1, 18, 18, 64, 64, 1): (32, 2, 1, True),
    (1, 25, 57, 64, 32, 1): (32, 1, 2, True), (4, 1, 40, 64, 32, 3): (64, 1, 1, True), (6, 7, 5, 32, 32, 3): (32, 1, 1, True)}
SPLIT_RESIDENT_REACHABLE = {(cs, nw, mt, r) for cs, nw, mt in ((32, 1, 1), (32, 2, 1), (32, 1, 2), (64, 1, 1)) for r in (False, True)}


def _split_plan(capfd, n, h, w, ci, co, kt, resident):
    head = 'split conv plan %s%dx%d %d->%d kt=%d n=%d:' % ('(resident) ' if resident else '', h, w, ci, co, kt, n)
    lines = _plan_lines(capfd, head)
    assert lines, 'no line "%s"' % head
    if resident:
        cs, nw, mt = (int(v) for v in re.search(r'cs=(\d+) nw=(\d+) mt=(\d+)', lines[-1]).groups())
        return cs, nw, mt, kt == 3 or ci != cs
    return tuple(int(v) for v in re.search(r'cs=(\d+) nw=(\d+) ngw=(\d+) mt=(\d+)', lines[-1]).groups())


def _split_forward_cases(n, frames, h, w, ci, co, kt, seed, families, light=False):
    """conv3x3_split: plain / bias + ReLU with want_amax for every family; on the first (dense) family the input mask, out_mask with and without
    the input mask, and the bf16 second output.  light (the largest shapes): one masked launch, input mask and out_mask together."""
    for fam in families:
        x, wt, b, code = _family(fam, seed, n, h, w, ci, co, kt, frames)
        wps = native.conv3x3_split_prepare_weights(_f(wt))[0]
        bias = b is not None
        ref = _forward_ref(fam, seed, n, h, w, ci, co, kt, frames, bias, bias)
        y, amax = native.conv3x3_split(_f(x), wps, _f(b) if bias else None, frames, bias, want_amax=True)
        _same(y, ref, F32, '%s frames=%d' % (fam, frames), _explainer(x, frames, kt, code))
        assert float(amax.max()) == float(ref.abs().max()), '%s: reported maximum %r, exact %r' % (fam, float(amax.max()), float(ref.abs().max()))
    fam = families[0]
    x, wt, b, _ = _family(fam, seed, n, h, w, ci, co, kt, frames)
    wps = native.conv3x3_split_prepare_weights(_f(wt))[0]
    xm, om = R.relu_like_mask(seed + 2, x.shape), R.relu_like_mask(seed + 3, (n, h, w, co))
    if not light:
        y = native.conv3x3_split(_f(x), wps, None, frames, False, mask=_f(xm))
        _same(y, R.conv3x3(x, wt, None, frames, mask=xm), F32, '%s input mask' % fam)
    for m in ((xm,) if light else (None, xm)):
        y, amax = native.conv3x3_split(_f(x), wps, None, frames, False, mask=_f(m) if m is not None else None, want_amax=True, out_mask=_f(om))
        ref = R.conv3x3(x, wt, None, frames, mask=m, out_mask=om)
        _same(y, ref, F32, '%s out_mask (input mask %s)' % (fam, m is not None))
        assert float(amax.max()) == float(ref.abs().max())
    y, amax, y16 = native.conv3x3_split(_f(x), wps, _f(b), frames, True, want_amax=True, want_bf16=True)
    ref = _forward_ref(fam, seed, n, h, w, ci, co, kt, frames, True, True)
    _same(y, ref, F32, '%s dual f32' % fam)
    _same(y16, ref, BF16, '%s dual bf16' % fam)
    assert float(amax.max()) == float(ref.abs().max())


@gpu
@pytest.mark.parametrize('shape', sorted(SPLIT_TILED))
def test_split_tiled_forward(shape, switches, capfd):
    n, h, w, ci, co = shape
    assert native.conv3x3_split_supported(h, w, ci, co)
    switches(PCACC_CONV_PLAN='1', PCACC_CONV_RES='0')
    capfd.readouterr()
    big = n * h * w * co > 1500000
    _split_forward_cases(n, 1, h, w, ci, co, 1, ci + h, ('dense', 'lo_x', 'lo_w') if big else ('dense', 'position', 'lo_x', 'lo_w'), light=big)
    assert _split_plan(capfd, n, h, w, ci, co, 1, False) == SPLIT_TILED[shape]


@gpu
@pytest.mark.parametrize('shape', sorted(SPLIT_RESIDENT))
def test_split_resident_forward(shape, switches, capfd):
    n, h, w, ci, co, kt = shape
    frames = 2 if kt == 3 and n == 4 else 3 if kt == 3 else 1
    switches(PCACC_CONV_PLAN='1', PCACC_CONV_RES='2')
    capfd.readouterr()
    _split_forward_cases(n, frames, h, w, ci, co, kt, ci + h + kt, ('dense', 'position', 'lo_x', 'lo_w'))
    assert _split_plan(capfd, n, h, w, ci, co, kt, True) == SPLIT_RESIDENT[shape]


@gpu
@pytest.mark.parametrize('n,frames,h,w,ci,co', [(2, 1, 9, 33, 32, 32), (4, 2, 7, 31, 32, 64), (6, 3, 8, 32, 64, 32), (2, 1, 17, 65, 64, 64), (6, 3, 1, 1, 32, 32)])
def test_split_3x3x3_tiled_forward(n, frames, h, w, ci, co, switches):
    """3x3x3 layers on the streaming kernel, two samples of 1 to 3 frames (a leak across the sample boundary shows in the position code)."""
    switches(PCACC_CONV_RES='0')
    _split_forward_cases(n, frames, h, w, ci, co, 3, ci + co + frames, ('dense', 'position', 'lo_x', 'lo_w'))


@gpu
def test_split_shapes_reach_every_reachable_variant(switches, capfd):
    """SPLIT_TILED / SPLIT_RESIDENT together reach every instantiated variant any shape with n <= 3, h, w <= 80, channels <= 512 reaches."""
    dev = _dev()
    seen = {'0': set(), '2': set()}
    for res, table in (('0', SPLIT_TILED), ('2', SPLIT_RESIDENT)):
        switches(PCACC_CONV_PLAN='1', PCACC_CONV_RES=res)
        capfd.readouterr()
        for shape in sorted(table):
            n, h, w, ci, co = shape[:5]
            kt = shape[5] if len(shape) > 5 else 1
            wps = (torch.zeros((2, 9 * kt, co, ci), dtype=torch.float16, device=dev), torch.ones((co,), device=dev))
            native.conv3x3_split(torch.zeros((n, h, w, ci), device=dev), wps, None, 2 if kt == 3 and n == 4 else 3 if kt == 3 else 1, False)
            torch.cuda.synchronize()
            seen[res].add(_split_plan(capfd, n, h, w, ci, co, kt, res == '2'))
    assert seen['0'] == SPLIT_TILED_REACHABLE and seen['2'] == SPLIT_RESIDENT_REACHABLE


@gpu
@pytest.mark.parametrize('n,h,w,ca,cb,co,res', [(2, 9, 33, 32, 32, 32, '0'), (2, 9, 33, 32, 32, 32, '2'), (1, 19, 37, 64, 64, 64, '0'), (1, 18, 18, 32, 96, 64, '0'),
                                                (1, 7, 5, 128, 128, 128, '0'), (2, 17, 31, 32, 32, 64, '2')])
def test_split_cat(n, h, w, ca, cb, co, res, switches):
    """conv3x3_split_cat at 32-aligned (32 + 32, 32 + 96) and 64-aligned (64 + 64, 128 + 128) channel boundaries == the convolution of the concatenation."""
    switches(PCACC_CONV_RES=res)
    for fam in ('dense', 'position', 'lo_x', 'lo_w'):
        x, wt, b, code = _family(fam, ca + h, n, h, w, ca + cb, co, 1, 1)
        a, bb = _f(x[..., :ca].contiguous()), _f(x[..., ca:].contiguous())
        amax = torch.maximum(native.absmax256(a), native.absmax256(bb))
        wps = native.conv3x3_split_prepare_weights(_f(wt))[0]
        bias = b is not None
        ref = R.conv3x3(x, wt, b, 1, relu=bias)
        y, ya, y16 = native.conv3x3_split_cat(a, bb, amax, wps, _f(b) if bias else None, bias, want_bf16=True)
        _same(y, ref, F32, fam, _explainer(x, 1, 1, code))
        _same(y16, ref, BF16, fam + ' bf16')
        assert float(ya.max()) == float(ref.abs().max())


SPLIT_WGRAD = [(2, 1, 7, 5, 32, 32, 1), (1, 1, 19, 37, 32, 64, 1), (1, 1, 33, 70, 64, 32, 1), (2, 1, 18, 18, 64, 64, 1), (1, 1, 1, 40, 128, 64, 1),
               (1, 1, 7, 5, 256, 128, 1), (6, 3, 9, 33, 32, 32, 3), (4, 2, 7, 31, 32, 64, 3), (2, 1, 5, 72, 96, 32, 1)]


@gpu
@pytest.mark.parametrize('n,frames,h,w,ci,co,kt', SPLIT_WGRAD)
def test_split_wgrad(n, frames, h, w, ci, co, kt):
    """conv3x3_wgrad_split with and without the ReLU mask; small integers, 20-bit dY against sparse signs and the mirror image."""
    for fam in ('small', 'lo_dy', 'lo_x'):
        g = torch.Generator().manual_seed(ci + co + h)
        if fam == 'small':
            x, gy = R.small_grad(ci + h, (n, h, w, ci)), R.small_grad(co + w, (n, h, w, co))
        else:                                                  # 20-bit dY (resp. X) against {-1,0,1}; the small operand (resp. dY) non-zero at 8 pixels: sums < 2^24
            px = torch.zeros((n * h * w, 1), dtype=torch.int64)
            px[torch.randint(0, n * h * w, (8,), generator=g)] = 1
            px = px.view(n, h, w, 1)
            if fam == 'lo_dy':
                gy = torch.randint(-(1 << 20) + 1, 1 << 20, (n, h, w, co), generator=g) * px
                x = torch.randint(-1, 2, (n, h, w, ci), generator=g)
            else:
                x = torch.randint(-(1 << 20) + 1, 1 << 20, (n, h, w, ci), generator=g)
                gy = torch.randint(-1, 2, (n, h, w, co), generator=g) * px
            assert R.lo_plane_bits(gy if fam == 'lo_dy' else x) > 0
        mask = R.relu_like_mask(h * w + 1, gy.shape)
        for m in (None, mask):
            dw_ref, db_ref = R.conv3x3_wgrad(gy, x, frames, kt, mask=m)
            md = _f(m) if m is not None else None
            if kt == 1:
                dw, db = native.conv3x3_wgrad_split(_f(gy), _f(x), mask=md)
                dw = dw.view(co, 3, 3, ci).permute(0, 3, 1, 2)
            else:
                parts = [native.conv3x3_wgrad_split(_f(gy), _f(x), frames, dt, mask=md) for dt in (-1, 0, 1)]
                dw = torch.stack([p[0].view(co, 3, 3, ci) for p in parts], 1).permute(0, 4, 1, 2, 3)
                db = parts[1][1]
            _same(dw, dw_ref, F32, '%s dW mask=%s' % (fam, m is not None))
            _same(db, db_ref, F32, '%s db mask=%s' % (fam, m is not None))


@gpu
@pytest.mark.parametrize('n,frames,h,w,ci,co,kt,res', [(2, 1, 9, 33, 32, 64, 1, '0'), (2, 1, 9, 33, 32, 64, 1, '2'), (6, 3, 7, 31, 32, 32, 3, '0'),
                                                       (4, 2, 7, 31, 64, 32, 3, '2'), (2, 1, 18, 18, 256, 128, 1, '0'), (1, 1, 19, 37, 128, 64, 1, '0')])
def test_split_autograd_path(n, frames, h, w, ci, co, kt, res, switches):
    """ops.set_split(True): y, dX, dW, db of ops.conv3x3_rows (conv + bias + ReLU), the ReLU mask taken from the reference."""
    switches(PCACC_CONV_RES=res)
    ops.set_split(True)
    x, wt, b, _ = _family('dense', ci + co + kt, n, h, w, ci, co, kt, frames)
    gy = R.small_grad(co + h, (n, h, w, co))
    xg, wg, bg = _f(x).requires_grad_(True), _f(wt).requires_grad_(True), _f(b).requires_grad_(True)
    y = ops.conv3x3_rows(xg, wg, bg, frames, True)
    y_ref = R.conv3x3(x, wt, b, frames, relu=True)
    _same(y, y_ref, F32, 'y')
    assert float(ops.amax_tag(y).max()) == float(y_ref.abs().max())
    y.backward(_f(gy))
    _same(xg.grad, R.conv3x3_dgrad(gy, wt, frames, mask=y_ref), F32, 'dX')
    dw_ref, db_ref = R.conv3x3_wgrad(gy, x, frames, kt, mask=y_ref)
    _same(wg.grad, dw_ref, F32, 'dW')
    _same(bg.grad, db_ref, F32, 'db')


# ---- transposed 2x2 convolution: fp32x3 and bf16 -------------------------------------------------------------------------------------------------
def _upconv_case(seed, n, h, w, ci, cu, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == 'small':
        x = torch.randint(-3, 4, (n, h, w, ci), generator=g)
        wt = torch.randint(-1, 2, (ci, cu, 2, 2), generator=g)
        gy = torch.randint(-3, 4, (n, 2 * h, 2 * w, cu), generator=g)
    elif kind == 'mantissa':                                   # bf16: all 8 significant bits, weights sparse signs
        x = torch.randint(-255, 256, (n, h, w, ci), generator=g)
        gy = torch.randint(-255, 256, (n, 2 * h, 2 * w, cu), generator=g)
        wt = torch.randint(-1, 2, (ci, cu, 2, 2), generator=g) * (torch.rand((ci, cu, 2, 2), generator=g) < 0.1)
    else:                                                      # fp32x3 lo planes: 20-bit activations and gradients, at most 8 weights per row and column
        x = torch.randint(-(1 << 20) + 1, 1 << 20, (n, h, w, ci), generator=g)
        gy = torch.randint(-(1 << 20) + 1, 1 << 20, (n, 2 * h, 2 * w, cu), generator=g)
        wt = torch.zeros((ci, cu, 2, 2), dtype=torch.int64)
        for k in range(2):
            perm = torch.randperm(max(ci, cu), generator=g)
            wt[torch.arange(max(ci, cu)) % ci, perm % cu, k, torch.randint(0, 2, (max(ci, cu),), generator=g)] = 1 - 2 * k
    b = torch.randint(-4, 5, (cu,), generator=g)
    return x, wt.to(torch.int64), b, gy


UPCONV = [(3, 5, 7, 64, 32), (2, 9, 9, 128, 64), (1, 1, 1, 64, 64), (2, 4, 6, 512, 256), (1, 17, 33, 64, 32)]


@gpu
@pytest.mark.parametrize('n,h,w,ci,cu', UPCONV)
def test_upconv2x2_split(n, h, w, ci, cu):
    assert native.upconv2x2_split_supported(h, w, ci, cu)
    for kind in ('small', 'lo'):
        x, wt, b, gy = _upconv_case(ci + h, n, h, w, ci, cu, kind)
        fwd, bwd = native.upconv2x2_split_prepare_weights(_f(wt))
        xa, ga = native.absmax256(_f(x)), native.absmax256(_f(gy))
        ref = R.upconv2x2(x, wt, b)
        y, ya = native.upconv2x2_split(_f(x), xa, fwd, _f(b), 0)
        _same(y, ref, F32, kind + ' forward')
        assert float(ya.max()) == float(ref.abs().max())
        y, ya, y16 = native.upconv2x2_split(_f(x), xa, fwd, _f(b), 0, want_bf16=True)
        _same(y, ref, F32, kind + ' forward (dual)')
        _same(y16, ref, BF16, kind + ' forward bf16')
        if kind == 'small':                                    # data and weight gradients sum over c_up resp. pixels: 20-bit operands would leave 2^24
            gx, gxa = native.upconv2x2_split(_f(gy), ga, bwd, None, 1)
            ref = R.upconv2x2_dgrad(gy, wt)
            _same(gx, ref, F32, 'data gradient')
            assert float(gxa.max()) == float(ref.abs().max())
            dw, db = native.upconv2x2_wgrad_split(_f(gy), ga, _f(x), xa)
            dw_ref, db_ref = R.upconv2x2_wgrad(gy, x)
            _same(dw, dw_ref, F32, 'dW')
            _same(db, db_ref, F32, 'db')


@gpu
@pytest.mark.parametrize('n,h,w,ci,cu', UPCONV)
def test_upconv2x2_bf16(n, h, w, ci, cu):
    """Forward, data gradient (dense and from a channel slice of a wider map: dy_pitch) and weight gradient (dense, and both operands sliced)."""
    assert native.upconv2x2_bf16_supported(ci, cu)
    dev = _dev()
    for kind in ('small', 'mantissa'):
        x, wt, b, gy = _upconv_case(ci + w, n, h, w, ci, cu, kind)
        fwd, bwd = native.upconv2x2_bf16_prepare_weights(_f(wt))
        _same(native.upconv2x2_bf16(_bf(x), fwd, _f(b), 0), R.upconv2x2(x, wt, b), BF16, kind + ' forward')
        _same(native.upconv2x2_bf16(_bf(x), fwd, None, 0), R.upconv2x2(x, wt, None), BF16, kind + ' forward, no bias')
        if kind == 'mantissa':
            gy = gy.clamp(-3, 3)                               # gradients sum over pixels: keep them small
        gx_ref = R.upconv2x2_dgrad(gy, wt)
        dw_ref, db_ref = R.upconv2x2_wgrad(gy, x)
        wide = torch.full((n, 2 * h, 2 * w, 2 * cu), 7.0, dtype=BF16, device=dev)      # the other half must never be read
        wide[..., cu:] = _bf(gy)
        xwide = torch.full((n, h, w, 2 * ci), 5.0, dtype=BF16, device=dev)
        xwide[..., :ci] = _bf(x)
        assert wide[..., cu:].stride(2) == 2 * cu and xwide[..., :ci].stride(2) == 2 * ci      # read in place through the pixel pitch
        for gin, xin, what in ((_bf(gy), _bf(x), 'dense'), (wide[..., cu:], xwide[..., :ci], 'sliced')):
            _same(native.upconv2x2_bf16(gin, bwd, None, 1), gx_ref, BF16, '%s data gradient (%s)' % (kind, what))
            dw, db = native.upconv2x2_bf16_wgrad(gin, xin, want_bias=True)
            _same(dw, dw_ref, F32, '%s dW (%s)' % (kind, what))
            _same(db, db_ref, F32, '%s db (%s)' % (kind, what))


# ---- the fg / bg head's last layer (csrc/head_conv.hip) ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('n,h,w,ci,co', [(2, 9, 33, 32, 1), (1, 17, 65, 64, 2), (3, 7, 31, 32, 4), (1, 1, 1, 32, 2), (2, 37, 53, 64, 4)])
def test_head_conv3x3(n, h, w, ci, co, dtype):
    assert native.head_conv3x3_supported(ci, co)
    put = _f if dtype == F32 else _bf
    for fam in ('dense', 'position') + (('lo_x',) if dtype == F32 else ('mantissa',)):
        x, wt, b, code = _family(fam, ci + h + co, n, h, w, ci, co, 1, 1)
        y = native.head_conv3x3_forward(put(x), _f(wt), _f(b) if b is not None else None)
        _same(y, R.conv3x3(x, wt, b), F32, fam + ' forward', _explainer(x, 1, 1, code))
    x, wt, b, _ = _family('dense', ci + h + co, n, h, w, ci, co, 1, 1)
    gy = R.small_grad(h + co, (n, h, w, co), -127, 127)
    _same(native.head_conv3x3_dgrad(_f(gy), _f(wt), ci, dtype), R.conv3x3_dgrad(gy, wt), dtype, 'data gradient')
    wcl = _f(wt).contiguous(memory_format=torch.channels_last)                           # the layout the model keeps the weight in
    _same(native.head_conv3x3_dgrad(_f(gy), wcl, ci, dtype), R.conv3x3_dgrad(gy, wt), dtype, 'data gradient, channels-last weight')
    dw, db = native.head_conv3x3_wgrad(_f(gy), put(x))
    dw_ref, db_ref = R.conv3x3_wgrad(gy, x)
    _same(dw, dw_ref, F32, 'dW')
    _same(db, db_ref, F32, 'db')
