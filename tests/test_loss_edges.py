"""The segmentation and offset loss kernels (csrc/loss.hip through ops.seg_loss / ops.offset_loss) against the float64 restatement
tests/loss_reference.py, on input families that each sit on one branch point of the kernels: the tile size of the rank scans, more tiles than one
block's stride, an absent class, no labelled row at all, the clamp of the class weights, massive ties, saturated probabilities; for the offsets the
switch from the LDS table to global atomics, label bases, one-point instances, far coordinates and rows placed exactly on the kinks of |x| and ||x||.

The rule.  With R64 the restatement and O the float32 formulation of the reference (oracle.seg_loss / oracle.offset_loss, pinned to the reference's own
outputs by tests/golden/loss.npz), every comparison asserts
    max |kernel - R64|  <=  4 * max |O - R64| + floor,      floor = FLOOR_ULPS float32 ulps of the quantity's magnitude
(loss values: max(1, |value|); offset_gt: the largest coordinate; gradients: their largest entry).  The same rule holds the oracle's CPU twin
(oracle/cpu_backend.py through ops.*) in the CPU part.  bf16 logit gradients are compared with the float64 gradient rounded to bf16, to one bf16 ulp of
the largest entry.  Exact contracts are asserted exactly: the IoU counters, zero gradients outside the selected rows, NaN / 0 / 0 when every row is
ignored, bit-equal offsets and zero L1 gradients on the dyadic family, and bit-equal results of two runs.  No row is excused anywhere: the families
keep distinct errors MIN_GAP apart and the offset estimates 0.05 m from the ground truth, or put them on the kink exactly.

Ties.  The Lovasz gradient of a row depends on the order inside a group of equal errors; the loss value does not.  What does not depend on the order is
the sum of the Jaccard gradients (dL/d error = the magnitude of dL/dp_c) over a tie group -- it telescopes to the Jaccard index after the group minus
the one before it.  (The signed sum of dL/dp_c does depend on the order: one foreground and one background row at intersection I, union U give
(I - U - 2) / (U (U + 1)) in one order and (I - U) / (U (U + 1)) in the other.)  The tie families are therefore held by these group sums, read from the
kernel's per-row Jaccard gradients (native.seg_loss_forward, the array the backward pass consumes); with no ignored row the groups of both classes
coincide and the same sums follow from the logit gradients alone, D_i = dL/dz0 / (p0 p1) = +-(g0 + g1) / 2, which `ties_labelled` asserts.  Per row the
kernel matches the stable-by-row-position order on `equal_logits` (asserted), where 1 - 0.5 = 0.5 is exact; on `ties` and `many_tiles` it need not: in
float32 1 - fl(p) and fl(1 - p) differ by an ulp, so the float32 sort separates foreground from background rows that tie in exact arithmetic.

Measured (MI355X and this file's CPU part; float32 ulps of the quantity's magnitude, the largest over the family's cases and quantities; `need` is the
largest (Ek - 4 Eref) on either the CPU twin or the GPU, i.e. what the floor has to cover):

    family         | values: Eref    GPU   twin | per-row gradients: Eref     GPU | tie-group sums: Eref    GPU | bf16 grads, GPU (bf16 ulp) | need
    tile_edges     |         0.45   0.55   0.47 |                  4593.2  4593.2 |                  -      -   |  1.00                      | 0.42
    many_tiles     |         0.06   0.40   0.40 |                     1.3     1.5 |              38.12  38.12   |  0.00                      | 0.16
    only_0         |         0.01   0.37   0.37 |                  1417.2  1417.2 |                  -      -   |  0.50                      | 0.36
    only_1         |         0.01   0.46   0.46 |                  1364.9  1364.9 |                  -      -   |  0.50                      | 0.41
    one_valid_row  |         0.28   0.28   0.28 |                     2.8     2.8 |                  -      -   |  0.00                      | 0.00
    clamped_1      |         0.07   0.33   0.33 |                  7284.2  7284.2 |                  -      -   |  1.00                      | 0.32
    clamped_0      |         0.05   0.41   0.41 |                  8823.5  8823.5 |                  -      -   |  0.50                      | 0.33
    ties           |         0.31   0.33   0.33 |                     1.3     1.3 |               1.84   1.84   |  0.00                      | 0.20
    ties_labelled  |         0.37   0.32   0.32 |                     0.9     1.1 |               3.59   2.92   |  0.00                      | 0.09
    equal_logits   |         0.25   0.02   0.02 |                   503.1   503.1 |               0.00   0.00   |  0.50                      | 0.00
    saturated      |         0.12   0.32   0.32 |                  4546.5  4546.5 |                  -      -   |  1.00                      | 0.15
    random         |         0.51   0.57   0.57 |                  4818.6  4818.6 |                  -      -   |  1.00                      | 0.33
    lds_edge       |         0.57   0.57   0.57 |                    13.8    14.8 |                  -      -   |  -                         | 0.40
    two_samples    |         0.98   0.98   0.98 |                     2.2     2.4 |                  -      -   |  -                         | 0.35
    singletons     |         1.47   1.47   1.47 |                    13.0    13.5 |                  -      -   |  -                         | 0.05
    far            |         0.56   0.56   0.56 |                     0.4     0.9 |                  -      -   |  -                         | 0.35
    dyadic_kinks   |         0.00   0.23   0.23 |                     0.5     1.8 |                  -      -   |  -                         | 0.23
    one_row        |        13.67  13.67  13.67 |                    14.7    35.3 |                  -      -   |  -                         | 0.28

The floor.  Across all families the largest excess over 4 * Eref is 0.46 ulp on the twin and 0.40 ulp on the GPU -- the rounding of a float32 result
(half an ulp) where the oracle, which keeps its sums in float64, happens to be exact.  FLOOR_ULPS = 1: that half ulp and as much again for the device's
expf / logf / sqrtf.  The per-row Lovasz gradients are the one place where Eref is large (5e-4 of the largest entry at 6000 rows): the reference forms
the Jaccard gradient as a difference of float32 Jaccard indices near 1, each good to 6e-8, for a result of order 1 / n; the kernel does the same sum in
the same order and lands on the oracle's values.  The rows of tile_edges at n = 1 and one_row have a single entry, so theirs is that entry's error.

What the file catches, one build of csrc/loss.hip per change and one run of the GPU part each (failing cases of 156):
    the 50.f clamp of the class weights removed               4    clamped_1, clamped_0 (cross entropy, both types)
    t < tile -> t <= tile in the prefix of seg_lovasz_kernel   145  every family with a labelled row
    the r > 0 subtraction dropped                              133  every family with more than one row
    r0 + k < n -> <= in seg_tile_fg_kernel                     88   tile_edges (never n = 2048: no partial tile), ties, clamped, random, equal_logits
    argmax tie to class 1 (z1 >= z0)                           49   equal_logits, ties, many_tiles, saturated; bf16 cases with equal logit pairs
    ignored rows counted as class 0 in the cross entropy       119  every family with an ignored row, all_ignored among them
    e > 0.f ? ... : 0.f replaced by the division               1    dyadic_kinks (NaN on the est == 0 rows)
    sign of the L1 gradient from >=                            1    dyadic_kinks (the est == gt rows)
    use_lds threshold off by one entry (<= -> <)               0    not observable: both table paths add the same 64-bit integers, so every output is the
                                                                    same bits whichever path a launch takes; lds_edge runs k = 2047, 2048, 2049 on both sides
"""
import functools

import numpy as np
import pytest
import torch

import loss_reference as ref
import oracle
from oracle import cpu_backend as cpu

KEYS = ('intersection', 'union', 'pred_positives', 'gt_positives')
LAYOUTS = ('rows', 'planes', 'channels_last')


def _seg_cases():
    cases = [('tile_edges', n, bf16, subset, layout) for n in ref.TILE_EDGES for layout in LAYOUTS for bf16 in (False, True) for subset in (False, True)]
    cases += [(f, None, bf16, False, 'rows') for f in ref.SEG_FAMILIES + ('ties_labelled',) for bf16 in (False, True)]
    cases += [('ties', None, bf16, True, 'rows') for bf16 in (False, True)] + [('ties', None, True, False, 'planes')]
    return cases


def _seg_id(c):
    return '%s%s-%s-%s-%s' % (c[0], '' if c[1] is None else '-%d' % c[1], 'bf16' if c[2] else 'f32', 'subset' if c[3] else 'all', c[4])


SEG_CASES = _seg_cases()
seg_cases = pytest.mark.parametrize('case', SEG_CASES, ids=_seg_id)
offset_cases = pytest.mark.parametrize('name', ref.OFFSET_CASES)


@functools.lru_cache(maxsize=None)
def _seg_refs(family, n, bf16, subset):
    """(z, y, rows, selected z, selected y, R64, O): computed once per input, shared by the CPU and the GPU tests, never written to."""
    z, y, rows = ref.seg_case(family, n, bf16, subset)
    zs, ys = (z, y) if rows is None else (z[rows], y[rows])
    return z, y, rows, zs, ys, ref.seg_loss64(zs, ys), oracle.seg_loss(zs, ys)


@functools.lru_cache(maxsize=None)
def _offset_refs(name):
    c = ref.offset_case(name)
    fb = np.zeros(c['points'].shape[0], np.int64)
    fb[c['rows']] = 1
    bounds = np.cumsum((0,) + c['sizes'])
    motions = [c['inst_motion'][bounds[b]:bounds[b + 1]] for b in range(len(c['sizes']))]
    o = oracle.offset_loss(c['points'], c['time_indice'], c['inst_labels'], fb, c['ego'], motions, c['transformed_points'], c['offset_est'])
    return c, ref.offset_ref(c), o


def _laid_out(z, layout, subset, dtype, dev):
    """The [n_total,2] logits as a leaf tensor of the layout."""
    t = torch.from_numpy(np.array(z)).to(dtype)
    if layout != 'rows':
        f, h, w = ref.planes_shape(z.shape[0], subset)
        t = t.view(f, h, w, 2)
        t = t.permute(0, 3, 1, 2).contiguous().to(dev) if layout == 'planes' else t.to(dev).permute(0, 3, 1, 2)   # NCHW shape either way
    else:
        t = t.to(dev)
    return t.requires_grad_(True)


def _as_rows(g, layout):
    g = g.detach().float().cpu().numpy().astype(np.float64)
    return g if layout == 'rows' else np.transpose(g, (0, 2, 3, 1)).reshape(-1, 2)


def _run_seg(ops, case, dev):
    family, n, bf16, subset, layout = case
    z, y, rows = _seg_refs(family, n, bf16, subset)[:3]
    est = _laid_out(z, layout, subset, torch.bfloat16 if bf16 else torch.float32, dev)
    terms, metric = ops.seg_loss(est, torch.from_numpy(np.array(y)).to(dev), None if rows is None else torch.from_numpy(np.array(rows)).to(dev))
    grads = [torch.autograd.grad(terms[k], est, retain_graph=True)[0] for k in range(2)]
    return est, terms.detach().cpu(), metric.cpu(), grads


def _same_bits(a, b):
    flat = lambda t: torch.empty(t.numel(), dtype=t.dtype, device=t.device).copy_(t.reshape(-1)).view(torch.uint8)   # NaN compares by its bits
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(flat(a), flat(b)))


def _check_seg(leg, case, terms, metric, grads):
    """The rule on the values, the counters and the per-row gradients of one segmentation case.  grads: [n_total,2] float64 per term."""
    family, n, bf16, subset, layout = case
    z, y, rows, zs, ys, r64, o = _seg_refs(family, n, bf16, subset)
    name = '%s %s' % (leg, _seg_id(case))
    terms = np.asarray(terms, np.float64)
    metric = np.asarray(metric, np.float64)
    assert np.array_equal(np.rint(metric * 1e3).astype(np.int64), r64['counts']), name
    assert np.abs(metric - r64['counts'] / 1e3).max() <= 1e-12, name
    sel = np.arange(z.shape[0]) if rows is None else rows
    outside = np.ones(z.shape[0], bool)
    outside[sel] = False
    for g in grads:
        assert np.isfinite(g).all() and not g[outside].any(), name              # exactly zero outside the selected rows
    if family == 'all_ignored':                                                 # torch's contract: value NaN, gradient 0; the predicted counts are not 0
        assert np.isnan(terms[0]) and np.isnan(r64['ce']) and np.isnan(o['bce_loss']), name
        assert terms[1] == 0 and r64['lovasz'] == 0 and not r64['counts'][0].any() and not r64['counts'][3].any(), name
        assert not grads[0].any() and not grads[1].any(), name
        return
    ref.check(name + ' ce', terms[0], o['bce_loss'], r64['ce'], scale=max(1.0, abs(r64['ce'])))
    ref.check(name + ' lovasz', terms[1], o['lovasz_loss'], r64['lovasz'], scale=1.0)
    per_row = [('grad_ce', grads[0][sel], o['grad_bce'], r64['grad_ce'])]
    if family not in ref.TIE_FAMILIES + ('ties_labelled',) or family == 'equal_logits':
        per_row.append(('grad_lovasz', grads[1][sel], o['grad_lovasz'], r64['grad_lovasz']))
    for key, got, want32, want in per_row:
        if bf16:
            worst = float(np.abs(got - ref.to_bf16(want)).max())
            print('LOSS-EDGES %-64s Ek %.3e  bf16 ulp %.3e' % (name + ' ' + key, worst, ref.ulp_bf16(np.abs(want).max())))
            assert worst <= ref.ulp_bf16(np.abs(want).max()), (name, key, worst)
        else:
            ref.check(name + ' ' + key, got, want32, want)
    if family == 'ties_labelled':
        # no ignored row: both classes' tie groups hold the same rows, and sum over a group of +-D_i, D_i = dL/dz0 / (p0 p1), is
        # (sum g0 + sum g1) / 2 whatever the order inside the group
        p = r64['p']
        sign = np.where(ys == 1, 1.0, -1.0) / (p[:, 0] * p[:, 1])
        sums = [ref.group_sums(g[:, 0] * sign, r64['order'][0], r64['starts'][0]) for g in (grads[1][sel], o['grad_lovasz'], r64['grad_lovasz'])]
        want = (ref.group_sums(r64['jaccard'][:, 0], r64['order'][0], r64['starts'][0]) + ref.group_sums(r64['jaccard'][:, 1], r64['order'][1], r64['starts'][1])) / 2
        assert all(np.array_equal(np.sort(r64['order'][0][a:b]), np.sort(r64['order'][1][a:b]))
                   for a, b in zip(r64['starts'][0][:-1], r64['starts'][0][1:])) and np.array_equal(r64['starts'][0], r64['starts'][1])
        assert np.abs(sums[2] - want).max() <= 1e-12 * np.abs(want).max()
        if bf16:
            # each stored gradient is within half a bf16 ulp of the float32 one; a group of s rows sums s such errors, scaled by 1 / (p0 p1)
            size = np.diff(r64['starts'][0])
            bound = ref.group_sums(np.abs(sign) * ref.ulp_bf16(np.abs(r64['grad_lovasz']).max()), r64['order'][0], r64['starts'][0])
            assert size.sum() == len(ys) and (np.abs(sums[0] - want) <= bound).all(), name
        else:
            ref.check(name + ' tie-group sums from the logit gradients', sums[0], sums[1], want)


def _check_jaccard(leg, case, jaccard):
    """Tie-group sums of the per-row Jaccard gradients [n,2] of one case."""
    family, n, bf16, subset, layout = case
    r64, o = _seg_refs(family, n, bf16, subset)[5:]
    for c in r64['present']:
        sums = [ref.group_sums(np.asarray(j)[:, c], r64['order'][c], r64['starts'][c]) for j in (jaccard, o['jaccard'], r64['jaccard'])]
        ref.check('%s %s tie-group sums class %d' % (leg, _seg_id(case), c), *sums)
        assert (np.asarray(jaccard)[:, c] >= 0).all()


# ---- CPU: the families are where they claim to be -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_seg_families_sit_on_their_branch_points(bf16):
    assert ref.SL_TILE - 1 in ref.TILE_EDGES and ref.SL_TILE in ref.TILE_EDGES and ref.SL_TILE + 1 in ref.TILE_EDGES and 6145 == 3 * ref.SL_TILE + 1
    for family, n, b, subset, layout in SEG_CASES:
        if b != bf16 or layout != 'rows':
            continue
        z, y, rows, zs, ys, r64, o = _seg_refs(family, n, b, subset)
        assert set(np.unique(y)) <= {-1, 0, 1} and (rows is None or (np.diff(rows) > 0).all() and rows[-1] < len(y) and rows[0] >= 0)
        assert not b or np.array_equal(ref.to_bf16(z), z.astype(np.float64))                       # the values are bf16 values
        tied = family in ref.TIE_FAMILIES + ('ties_labelled', 'saturated')
        if not tied:                                                                               # distinct errors, MIN_GAP apart, in either class
            for c in range(2):
                es = r64['err'][r64['order'][c], c]
                assert len(r64['starts'][c]) == len(ys) + 1 and (len(ys) < 2 or -np.diff(es).max() >= ref.MIN_GAP), (family, n)
                assert np.array_equal(np.argsort(-np.abs((ys == c) - _softmax32(zs)[:, c]), kind='stable'), r64['order'][c]), (family, n)   # float32 orders alike
    r = {f: _seg_refs(f, None, bf16, False) for f in ref.SEG_FAMILIES + ('ties_labelled',)}
    assert len(r['many_tiles'][4]) == 256 * ref.SL_TILE + 1
    assert set(r['only_0'][4]) == {-1, 0} and set(r['only_1'][4]) == {-1, 1} and set(r['all_ignored'][4]) == {-1} and len(r['only_0'][4]) == ref.SL_TILE + 1
    assert list(r['one_valid_row'][4]) == [-1, 1, -1] and -1 not in r['ties_labelled'][4]
    for family, rare in (('clamped_1', 1), ('clamped_0', 0)):                                       # the clamp is active, on the rare class only
        ys, r64 = r[family][4], r[family][5]
        assert (ys == rare).sum() == 2 and (ys == 1 - rare).sum() / 2 > 2500 and len(ys) == 6000
        assert r64['w_raw'][rare] > 50 and r64['w'][rare] == 50 and r64['w'][1 - rare] == r64['w_raw'][1 - rare] < 50
        assert family == 'clamped_1' or (ys == -1).sum() == 900
        assert oracle.ce_weights(ys)[rare] == 50
    for family, most in (('ties', 5), ('ties_labelled', 5), ('many_tiles', 65), ('equal_logits', 1)):
        ys, r64 = r[family][4], r[family][5]
        for c in range(2):
            starts, order = r64['starts'][c], r64['order'][c]
            assert len(starts) - 1 <= most
            for a, b_ in zip(starts[:-1], starts[1:]):                                             # every group mixes foreground, background and ignored rows
                assert {c, 1 - c} <= set(ys[order[a:b_]]) and (family == 'ties_labelled' or -1 in ys[order[a:b_]]), (family, c)
    ys, r64 = r['equal_logits'][4], r['equal_logits'][5]
    assert (r64['err'] == 0.5).all() and not r64['counts'][2, 1] and r64['counts'][2, 0] == len(ys)  # argmax tie -> class 0
    zs, ys, r64, o = r['saturated'][3:]
    d = np.abs(zs[:, 1].astype(np.float64) - zs[:, 0])
    p32 = _softmax32(zs)
    assert (d >= 110).sum() > 1000 and np.isin(p32[d >= 110], (0.0, 1.0)).all() and np.isin(r64['p'][d > 800], (0.0, 1.0)).all()
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in (r64['ce'], r64['lovasz'], r64['grad_ce'], r64['grad_lovasz'], o['bce_loss'], o['grad_bce']))
    assert np.log(np.maximum(r64['p'], 1e-300)).min() < -600 and (zs.min(), zs.max()) == ((-9984, 9984) if bf16 else (-1e4, 1e4))


def _softmax32(zs):
    """The float32 softmax of the oracle (oracle.seg_loss's own lines)."""
    z = np.asarray(zs, np.float32)
    ez = np.exp(z - z.max(1, keepdims=True))
    return (ez / ez.sum(1, keepdims=True)).astype(np.float32)


def test_offset_families_sit_on_their_branch_points():
    ks = {}
    for name in ref.OFFSET_CASES:
        c, r64, o = _offset_refs(name)
        n, k = c['points'].shape[0], c['inst_motion'].shape[0]
        ks[name] = k
        lab = c['inst_labels'] + c['label_base'][c['time_indice'][:, 0]]
        assert k == sum(c['sizes']) and lab.min() >= 0 and lab.max() < k and (np.diff(c['rows']) > 0).all() and c['rows'][-1] < n
        assert all(c['inst_labels'][c['time_indice'][:, 0] == b].max() < s for b, s in enumerate(c['sizes']))
        assert c['time_indice'][:, 1].max() < c['ego'].shape[1] == c['inst_motion'].shape[1]
        rot = c['inst_motion'][..., :3, :3].astype(np.float64)
        assert np.abs(rot @ np.swapaxes(rot, -1, -2) - np.eye(3)).max() < 1e-6                       # rigid
        if name != 'dyadic_kinks':                                                                 # estimates clear of the kink of |gt - est|
            assert np.abs(r64['offset_gt'] - c['offset_est'][c['rows']]).min() >= 0.049 and np.abs(c['offset_est'][c['rows']]).min() > 0
    assert ks['lds_edge-2047'] * 3 < ref.OFF_LDS_ENTRIES == ks['lds_edge-2048'] * 3 < ks['lds_edge-2049'] * 3
    c = ref.offset_case('two_samples')
    assert list(c['label_base']) == [0, 1500] and ks['two_samples'] * 3 > ref.OFF_LDS_ENTRIES
    assert (c['inst_labels'][c['time_indice'][:, 0] == 1] + 1500).max() >= ref.OFF_LDS_ENTRIES // 3
    c = ref.offset_case('singletons')
    assert np.array_equal(np.bincount(c['inst_labels'], minlength=4096), np.ones(4096, np.int64))
    assert len(np.setdiff1d(np.arange(4096), c['inst_labels'][c['rows']])) > 1000                   # labels in the table that carry no selected row
    c = ref.offset_case('far')
    assert np.abs(c['points']).min(0).max() > 1500 and (c['points'] > 0).any() and (c['points'] < 0).any()
    assert len(ref.offset_case('one_row')['rows']) == 1


def test_dyadic_family_is_exact_in_both_precisions():
    c, r64, o = _offset_refs('dyadic_kinks')
    gt, est, kind = r64['offset_gt'], c['offset_est'][c['rows']].astype(np.float64), c['kind'][c['rows']]
    assert np.array_equal(gt * 16, np.rint(gt * 16)) and np.array_equal(o['offset_gt'].astype(np.float64), gt)   # float32 arithmetic gives the same bits
    assert np.array_equal(np.bincount(c['inst_labels'] + c['label_base'][c['time_indice'][:, 0]]), np.full(64, 16))
    assert [(kind == q).sum() for q in range(4)] == [192, 192, 96, 288]
    assert (est[kind == 0] == gt[kind == 0]).all() and not est[kind == 1].any() and (gt[kind == 1] != 0).all()
    assert not gt[kind == 2].any() and (est[kind == 2] != 0).all() and (est[kind == 3] != gt[kind == 3]).all() and (gt[kind == 3] != 0).all()
    g = r64['grad_norm'][c['rows']]
    assert not g[kind == 0].any() and (np.abs(g[kind != 0]) == 1 / 768).all()
    assert np.isfinite(r64['grad_dir']).all() and np.abs(r64['grad_dir'][c['rows']][kind == 1]).max() > 1e15    # the u / 1e-20 rows


# ---- CPU: the oracle and its twin against float64 -------------------------------------------------------------------------------------------
@seg_cases
def test_oracle_and_twin_seg_loss_against_float64(case, monkeypatch):
    family, n, bf16, subset, layout = case
    z, y, rows, zs, ys, r64, o = _seg_refs(family, n, bf16, subset)
    full = lambda g: _scatter(g, rows, z.shape[0])
    _check_seg('oracle', case, (o['bce_loss'], o['lovasz_loss']), np.stack([o['metric'][k] for k in KEYS]), [full(o['grad_bce']), full(o['grad_lovasz'])])
    if family in ref.TIE_FAMILIES:
        _check_jaccard('oracle', case, o['jaccard'])
    from pcaccumulation_amd import ops
    cpu.install(monkeypatch)
    est, terms, metric, grads = _run_seg(ops, case, torch.device('cpu'))
    _check_seg('twin', case, terms.numpy(), metric.numpy(), [_as_rows(g, layout) for g in grads])


def _scatter(g, rows, n_total):
    if rows is None:
        return np.asarray(g, np.float64)
    out = np.zeros((n_total, 2))
    out[rows] = g
    return out


def _offset_tensors(c, dev):
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return [t(c[k]) for k in ('points', 'time_indice', 'inst_labels', 'label_base', 'ego', 'inst_motion', 'transformed_points', 'rows')]


def _run_offset(ops, name, dev):
    c = ref.offset_case(name)
    e = torch.from_numpy(np.array(c['offset_est'])).to(dev).requires_grad_(True)
    out, gt = ops.offset_loss(e, *_offset_tensors(c, dev))
    grads = [torch.autograd.grad(out[k], e, retain_graph=True)[0] for k in range(3)]
    return out.detach().cpu(), gt.cpu(), [g.cpu() for g in grads]


def _check_offset(leg, name, out, gt, grads):
    c, r64, o = _offset_refs(name)
    rows = c['rows']
    out, gt = out.numpy().astype(np.float64), gt.numpy().astype(np.float64)
    g_norm, g_dir, g_l2 = (g.numpy().astype(np.float64) for g in grads)
    tag = '%s %s' % (leg, name)
    for k, (key, okey) in enumerate((('norm', 'offset_norm_loss'), ('dir', 'offset_dir_loss'), ('l2', 'offset_l2_error'))):
        ref.check('%s %s' % (tag, key), out[k], o[okey], r64[key], scale=max(1.0, abs(r64[key])))
    coord = max(np.abs(c['points']).max(), np.abs(c['transformed_points']).max())
    if name == 'dyadic_kinks':
        assert np.array_equal(gt, r64['offset_gt']), tag                                           # bit-equal
    ref.check(tag + ' offset_gt', gt, o['offset_gt'], r64['offset_gt'], scale=coord)
    outside = np.ones(c['points'].shape[0], bool)
    outside[rows] = False
    assert not g_l2.any() and not g_norm[outside].any() and not g_dir[outside].any(), tag          # the L2 error is reported, not trained on
    assert np.isfinite(g_norm).all() and np.isfinite(g_dir).all(), tag
    assert np.array_equal(np.sign(g_norm[rows]), np.sign(r64['grad_norm'][rows])), tag              # every row, the est == gt rows (sign 0) included
    ref.check(tag + ' grad_norm', g_norm, o['grad_norm'], r64['grad_norm'])
    zero_est = ~c['offset_est'][rows].any(1)                                                       # rows of magnitude u / 1e-20: entry by entry, relatively
    ref.check_relative(tag + ' grad_dir est == 0', g_dir[rows][zero_est], o['grad_dir'][rows][zero_est], r64['grad_dir'][rows][zero_est])
    ref.check(tag + ' grad_dir', g_dir[rows][~zero_est], o['grad_dir'][rows][~zero_est], r64['grad_dir'][rows][~zero_est])


@offset_cases
def test_oracle_and_twin_offset_loss_against_float64(name, monkeypatch):
    c, r64, o = _offset_refs(name)
    t = torch.from_numpy
    _check_offset('oracle', name, t(np.array([o['offset_norm_loss'], o['offset_dir_loss'], o['offset_l2_error']])), t(o['offset_gt']),
                  [t(o['grad_norm']), t(o['grad_dir']), torch.zeros(c['points'].shape[0], 2)])
    from pcaccumulation_amd import ops
    cpu.install(monkeypatch)
    _check_offset('twin', name, *_run_offset(ops, name, torch.device('cpu')))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gpu_ops():
    from pcaccumulation_amd import native, ops as o
    native.lib()
    return o


@pytest.mark.gpu
@seg_cases
def test_seg_loss_kernels_against_float64(gpu_ops, dev, case):
    family, n, bf16, subset, layout = case
    est, terms, metric, grads = _run_seg(gpu_ops, case, dev)
    _, terms2, metric2, grads2 = _run_seg(gpu_ops, case, dev)
    assert _same_bits(terms, terms2) and _same_bits(metric, metric2) and all(_same_bits(a, b) for a, b in zip(grads, grads2))
    _check_seg('gpu', case, terms.numpy(), metric.numpy(), [_as_rows(g, layout) for g in grads])
    if family in ref.TIE_FAMILIES:
        from pcaccumulation_amd import native
        z, y, rows = _seg_refs(family, n, bf16, subset)[:3]
        plane = 0 if layout == 'rows' else est.shape[-1] * est.shape[-2]
        r = None if rows is None else torch.from_numpy(np.array(rows)).to(dev)
        lov = native.seg_loss_forward(est.detach(), plane, torch.from_numpy(np.array(y)).to(dev), r, z.shape[0] if rows is None else len(rows))[2]
        _check_jaccard('gpu', case, lov.cpu().numpy().T)


@pytest.mark.gpu
@offset_cases
def test_offset_loss_kernels_against_float64(gpu_ops, dev, name):
    out, gt, grads = _run_offset(gpu_ops, name, dev)
    out2, gt2, grads2 = _run_offset(gpu_ops, name, dev)
    assert _same_bits(out, out2) and _same_bits(gt, gt2) and all(_same_bits(a, b) for a, b in zip(grads, grads2))
    _check_offset('gpu', name, out, gt, grads)
    if name == 'dyadic_kinks':
        c, r64, _ = _offset_refs(name)
        kind = c['kind'][c['rows']]
        assert not grads[0].numpy()[c['rows']][kind == 0].any()                                    # est == gt: the L1 gradient is exactly 0
