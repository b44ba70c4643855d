"""Float64 restatement, in plain numpy, of the two loss passes of csrc/loss.hip -- the two-class segmentation loss (libs/loss.py:90-137: class-frequency
weighted cross entropy; libs/lovasz_softmax.py:56-94: Lovasz-Softmax; libs/loss.py:17-50: the IoU counters) and the offset loss (libs/loss.py:194-245) --
written from their definitions, with the gradients worked out by hand, for tests/test_loss_edges.py.  Also here: the yardstick of those tests and the
seeded input families, each built to sit on one branch point of the kernels.

Two choices make the float64 numbers the mathematical ones rather than a wider copy of the float32 ones.  The error of a foreground row, |1 - p_c|, is
formed as the probability of the other class, e_other / (e_0 + e_1), which is the same number without the cancellation; rows whose logit pairs are each
other's mirror image then tie bit for bit, as they do in exact arithmetic.  And the cumulative counts behind the Jaccard gradient are integers."""
import functools

import numpy as np

SL_TILE = 2048                                                                   # csrc/loss.hip
OFF_LDS_ENTRIES = 6144                                                           # csrc/loss.hip OFF_LDS_FLOATS: k * 3 <= this -> LDS table
MAX_WEIGHT = 50.0
EPS = 1e-20
MARGIN = 4.0
FLOOR_ULPS = 1                                                                   # how it was fixed: tests/test_loss_edges.py docstring


# ---- the restatement: segmentation ---------------------------------------------------------------------------------------------------------
def ce_weights64(y):
    """-> (w [2] float64, unclamped [2] float64).  Counts as float32 values + 1e-20 (libs/loss.py:97); ratio, sqrt and clamp in float64."""
    counts = np.array([np.float32((y == c).sum()) + np.float32(EPS) for c in range(2)], np.float32).astype(np.float64)
    raw = np.sqrt(counts.sum() / counts)
    return np.clip(raw, 0.0, MAX_WEIGHT), raw


def seg_loss64(z, y):
    """z [n,2]: the logits as the float32 / bf16 values they hold; y [n] in {-1, 0, 1}.  Returns a dict:
    ce, lovasz          the two terms (ce is NaN when every row is ignored, as torch's cross_entropy; lovasz is 0 then)
    counts [4,2] int64  intersection, union, predicted, labelled per class (the kernel reports them / 1e3)
    grad_ce, grad_lovasz [n,2]  gradients w.r.t. the logits (all zero where the term does not depend on them)
    p [n,2], w [2], w_raw [2]
    jaccard [n,2]       per row and class the Jaccard gradient of its rank (errors descending, ties in row order); 0 for an absent class
    err [n,2], order [2][n], starts [2][groups+1]  the errors, their stable descending order and the tie groups: maximal runs of equal error are
                        order[c][starts[c][g]:starts[c][g+1]]."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y).astype(np.int64)
    n = z.shape[0]
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    logp = (z - m) - np.log(s)
    w, w_raw = ce_weights64(y)
    keep = y >= 0
    safe = np.where(keep, y, 0)
    rows = np.arange(n)
    wi = w[safe] * keep
    wsum = wi.sum()
    with np.errstate(invalid='ignore'):
        ce = -(wi * logp[rows, safe]).sum() / wsum                               # 0 / 0 when nothing is labelled
    grad_ce = np.zeros((n, 2))
    if wsum > 0:
        other = p[rows, 1 - safe]                                                # p_y - 1 = -p_other, without the cancellation
        grad_ce[rows, safe] = -other
        grad_ce[rows, 1 - safe] = other
        grad_ce *= (wi / wsum)[:, None]
    present = [c for c in range(2) if (y == c).any()]
    err, jac_rows, dprob = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    order, starts, losses = [None, None], [None, None], []
    for c in range(2):
        fg = y == c
        err[:, c] = np.where(fg, p[:, 1 - c], p[:, c])
        order[c] = np.argsort(-err[:, c], kind='stable')
        es = err[order[c], c]
        starts[c] = np.concatenate(([0], np.nonzero(np.diff(es) != 0)[0] + 1, [n])).astype(np.int64)
        if c not in present:
            continue
        fgs = fg[order[c]].astype(np.int64)
        gts = int(fgs.sum())
        jac = 1.0 - (gts - np.cumsum(fgs)) / (gts + np.cumsum(1 - fgs)).astype(np.float64)
        g = np.diff(jac, prepend=0.0)
        losses.append(float(np.dot(es, g)))
        jac_rows[order[c], c] = g
        sign = np.where(err[:, c] == 0, 0.0, np.where(fg, -1.0, 1.0))            # d|fg - p| / dp, 0 at 0 as torch.abs
        dprob[:, c] = jac_rows[:, c] * sign / len(present)
    d0 = p[:, 0] * p[:, 1] * (dprob[:, 0] - dprob[:, 1])                         # softmax Jacobian of two classes
    pred = z[:, 1] > z[:, 0]                                                     # argmax, ties -> class 0
    counts = np.zeros((4, 2), np.int64)
    for c in range(2):
        pc = pred == bool(c)
        counts[0, c], counts[2, c], counts[3, c] = (pc & (y == c)).sum(), pc.sum(), (y == c).sum()
    counts[1] = counts[2] + counts[3] - counts[0]
    return {'ce': float(ce), 'lovasz': float(np.mean(losses)) if losses else 0.0, 'counts': counts, 'grad_ce': grad_ce,
            'grad_lovasz': np.stack((d0, -d0), 1), 'p': p, 'w': w, 'w_raw': w_raw, 'jaccard': jac_rows, 'err': err, 'order': order, 'starts': starts,
            'present': present}


def group_sums(values, order, starts):
    """Sum of per-row values over each tie group."""
    return np.add.reduceat(np.asarray(values, np.float64)[order], starts[:-1])


# ---- the restatement: offsets --------------------------------------------------------------------------------------------------------------
def offset_loss64(points, time_indice, inst_labels, label_base, ego, inst_motion, transformed_points, offset_est, rows):
    """points [n,3], time_indice [n,2] (sample, frame), inst_labels [n] per-sample labels, label_base [samples], ego [samples,frames,4,4],
    inst_motion [k,frames,4,4] (all samples stacked), transformed_points [n,>=2], offset_est [n,2], rows [m] selected rows.  Returns a dict:
    norm, dir, l2 (the three values), offset_gt [m,2], grad_norm, grad_dir [n,2] (w.r.t. offset_est; sign(0) = 0 and d|v|/dv = 0 at v = 0)."""
    pts = np.asarray(points, np.float64)
    tidx = np.asarray(time_indice).astype(np.int64)
    lab = np.asarray(inst_labels).astype(np.int64) + np.asarray(label_base).astype(np.int64)[tidx[:, 0]]
    ego = np.asarray(ego, np.float64)
    mot = np.asarray(inst_motion, np.float64)
    rows = np.asarray(rows).astype(np.int64)
    a = ego[tidx[:, 0], tidx[:, 1]]
    comp = np.einsum('nij,nj->ni', a[:, :3, :3], pts) + a[:, :3, 3]
    b = mot[lab, tidx[:, 1]]
    rec = np.einsum('nij,nj->ni', b[:, :3, :3], comp) + b[:, :3, 3]
    k = mot.shape[0]
    sums = np.zeros((k, 2))
    np.add.at(sums, lab, rec[:, :2])
    centres = sums / np.maximum(np.bincount(lab, minlength=k), 1)[:, None]
    gt = centres[lab[rows]] - np.asarray(transformed_points, np.float64)[rows, :2]
    est = np.asarray(offset_est, np.float64)[rows]
    m = rows.shape[0]
    diff = gt - est
    gn, en = np.linalg.norm(gt, axis=1, keepdims=True), np.linalg.norm(est, axis=1, keepdims=True)
    ngt = gt / (gn + EPS)
    out = {'norm': float(np.abs(diff).mean(0).sum()), 'dir': float((1 - (ngt * est / (en + EPS)).sum(1)).mean()),
           'l2': float(np.linalg.norm(diff, axis=1).mean()), 'offset_gt': gt}
    grad_norm, grad_dir = np.zeros((pts.shape[0], 2)), np.zeros((pts.shape[0], 2))
    grad_norm[rows] = -np.sign(diff) / m
    with np.errstate(invalid='ignore', divide='ignore'):
        unit = np.where(en > 0, est / en, 0.0)
    grad_dir[rows] = -(ngt / (en + EPS) - (ngt * est).sum(1, keepdims=True) / (en + EPS) ** 2 * unit) / m
    out.update(grad_norm=grad_norm, grad_dir=grad_dir)
    return out


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def ulp_bf16(x):
    """Spacing of bf16 at |x|: 2^(exponent - 7)."""
    x = abs(float(x))
    return 0.0 if x == 0 else float(2.0 ** (np.floor(np.log2(x)) - 7))


def to_bf16(a):
    """float values rounded to the nearest bf16 (ties to even), returned as float64."""
    import torch
    return torch.from_numpy(np.array(a, np.float32)).to(torch.bfloat16).double().numpy()


MEASURED = []                                                                    # (name, Ek, Eref, floor) of every comparison of this process


def check(name, got, oracle, r64, scale=None):
    """max |got - r64| <= MARGIN * max |oracle - r64| + FLOOR_ULPS float32 ulps of `scale` (default: the largest |r64|).  The figures are printed
    before the assertion (pytest -s shows them)."""
    got, oracle, r64 = (np.asarray(a, np.float64) for a in (got, oracle, r64))
    if r64.size == 0:
        assert got.size == 0
        return
    ek, eref = float(np.abs(got - r64).max()), float(np.abs(oracle - r64).max())
    floor = FLOOR_ULPS * ulp32(np.abs(r64).max() if scale is None else scale)
    line = 'LOSS-EDGES %-64s Ek %.3e  Eref %.3e  floor %.3e' % (name, ek, eref, floor)
    print(line)
    MEASURED.append((name, ek, eref, floor))
    assert np.isfinite(r64).all() and np.isfinite(eref), line
    assert np.isfinite(ek) and ek <= MARGIN * eref + floor, line


def check_relative(name, got, oracle, r64):
    """The same rule entry by entry, relative to each entry of r64 (for entries of very different magnitude: the u / 1e-20 rows)."""
    got, oracle, r64 = (np.asarray(a, np.float64) for a in (got, oracle, r64))
    nz = r64 != 0
    assert np.array_equal(got[~nz], r64[~nz]), name
    if nz.any():
        check(name, got[nz] / r64[nz], oracle[nz] / r64[nz], np.ones(int(nz.sum())))


# ---- input families: segmentation ----------------------------------------------------------------------------------------------------------
TILE_EDGES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 6145)
SEG_FAMILIES = ('many_tiles', 'only_0', 'only_1', 'all_ignored', 'one_valid_row', 'clamped_1', 'clamped_0', 'ties', 'equal_logits', 'saturated', 'random')
TIE_FAMILIES = ('ties', 'equal_logits', 'many_tiles')                            # Lovasz gradients held by tie-group sums
MIN_GAP = 4e-6                                                                   # between distinct errors; a float32 probability is good to ~1e-7


def _as(z, bf16):
    z = np.asarray(z, np.float32)
    return to_bf16(z).astype(np.float32) if bf16 else z


def _gaps_ok(z, y):
    """Rows whose error, for either class, is closer than MIN_GAP to the next one: there float32 and float64 could order the rows differently."""
    r = seg_loss64(z, y)
    bad = np.zeros(len(y), bool)
    for c in range(2):
        o = r['order'][c]
        close = np.nonzero(-np.diff(r['err'][o, c]) < MIN_GAP)[0]
        bad[o[close + 1]] = True
    return bad


def separated_logits(rs, n, y, bf16, scale=3.0):
    """randn * scale in the logits' type; rows with an error within MIN_GAP of another row's are drawn again, so the order of the errors -- and
    with it every row's Jaccard gradient -- is the same in float32 and float64 and no row has to be excused."""
    z = _as(rs.randn(n, 2) * scale, bf16)
    for _ in range(200):
        bad = _gaps_ok(z, y)
        if not bad.any():
            return z
        z[bad] = _as(rs.randn(int(bad.sum()), 2) * scale, bf16)
    raise AssertionError('no separated logits for n = %d' % n)


def _labels(rs, n, p_ignore=0.1, p_one=0.3):
    u = rs.rand(n)
    return np.where(u < p_ignore, -1, np.where(u < p_ignore + p_one, 1, 0)).astype(np.int64)


def mirrored_logits(rs, n, values, bf16):
    """Rows (a, -a) with a from `values` (exact in bf16): the errors of either class take at most len(values) distinct values, each shared by
    foreground, background and ignored rows."""
    a = rs.choice(np.asarray(values, np.float32), n)
    return _as(np.stack((a, -a), 1), bf16)


@functools.lru_cache(maxsize=None)
def seg_case(family, n=None, bf16=False, subset=False):
    """-> (z [n_total,2] float32 holding values of the logits' type, y [n_total], rows [n] or None).  With subset the supervised rows are a strictly
    increasing subset of 12 * W >= 4 n / 3 rows (planes of 4 x W cells, 3 frames); the family is what the selected rows show."""
    rs = np.random.RandomState((sum(map(ord, family)) * 7919 + (n or 0) * 31 + bf16 * 3 + subset) % (2 ** 31))
    if family == 'tile_edges':
        y = _labels(rs, n)
        y[rs.randint(n)] = 1 if n > 1 else 0
        z = separated_logits(rs, n, y, bf16)
    elif family == 'many_tiles':
        n = 256 * SL_TILE + 1
        y = _labels(rs, n)
        z = mirrored_logits(rs, n, np.arange(-32, 33) / 8.0, bf16)
    elif family in ('only_0', 'only_1', 'all_ignored'):
        n = SL_TILE + 1
        y = _labels(rs, n)
        y[y >= 0] = {'only_0': 0, 'only_1': 1, 'all_ignored': -1}[family]
        z = separated_logits(rs, n, y, bf16)
    elif family == 'one_valid_row':
        n, y = 3, np.array([-1, 1, -1], np.int64)
        z = separated_logits(rs, n, y, bf16)
    elif family in ('clamped_1', 'clamped_0'):
        n = 6000
        rare = int(family[-1])
        y = np.full(n, 1 - rare, np.int64)
        if rare == 0:
            y[rs.choice(n, 900, replace=False)] = -1
        y[rs.choice(np.nonzero(y >= 0)[0], 2, replace=False)] = rare
        z = separated_logits(rs, n, y, bf16)
    elif family in ('ties', 'ties_labelled'):                                    # ties_labelled: no ignored row, the tie groups of both classes coincide
        n = 6000
        y = _labels(rs, n, p_ignore=0.2 if family == 'ties' else 0.0, p_one=0.4)
        z = mirrored_logits(rs, n, (-2, -1, 0, 1, 2), bf16)
    elif family == 'equal_logits':
        n = SL_TILE + 1
        y = _labels(rs, n)
        z = _as(np.repeat(rs.choice(np.arange(-8, 9) / 4.0, n)[:, None], 2, 1), bf16)
    elif family == 'saturated':
        n = 6000
        y = _labels(rs, n)
        z = _as(rs.choice(np.array([-1e4, -90, -20, 0, 20, 90, 1e4], np.float32), (n, 2)), bf16)
    else:
        assert family == 'random', family
        n = 6000
        y = _labels(rs, n)
        z = separated_logits(rs, n, y, bf16)
    if not subset:
        return _frozen(z, y, None)
    n_total = 12 * ((n + n // 3 + 5 + 11) // 12)
    rows = np.sort(rs.choice(n_total, n, replace=False)).astype(np.int64)
    zt, yt = _as(rs.randn(n_total, 2) * 3, bf16), _labels(rs, n_total)
    zt[rows], yt[rows] = z, y
    return _frozen(zt, yt, rows)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)                                              # shared between tests: left unchanged
    return arrays


def planes_shape(n_total, subset):
    """(F, H, W) with F * H * W = n_total: (3, 4, W) for the subset cases, else the smallest prime factor of n_total as F and one row of cells."""
    if subset:
        return 3, 4, n_total // 12
    f = next((d for d in range(2, int(n_total ** 0.5) + 1) if n_total % d == 0), 1)
    return f, 1, n_total // f


# ---- input families: offsets ---------------------------------------------------------------------------------------------------------------
OFFSET_CASES = ('lds_edge-2047', 'lds_edge-2048', 'lds_edge-2049', 'two_samples', 'singletons', 'far', 'dyadic_kinks', 'one_row', 'random')


def _rigid(rs, shape, shift):
    """Random rotations (unit quaternions) and translations, float32 4x4."""
    q = rs.randn(*shape, 4)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = np.moveaxis(q, -1, 0)
    r = np.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), -1).reshape(*shape, 3, 3)
    m = np.zeros(tuple(shape) + (4, 4), np.float32)
    m[..., :3, :3] = r
    m[..., :3, 3] = rs.randn(*shape, 3) * shift
    m[..., 3, 3] = 1
    return m


@functools.lru_cache(maxsize=None)
def offset_case(name):
    """-> dict of float32 / int64 arrays: points, time_indice, inst_labels (per sample), label_base, sizes, ego, inst_motion (stacked),
    transformed_points, offset_est, rows, and for dyadic_kinks the row classes 'kind' (0 est == gt, 1 est == 0, 2 gt == 0, 3 ordinary)."""
    rs = np.random.RandomState(sum(map(ord, name)) * 104729 % (2 ** 31))
    spread, kind = 20.0, None
    if name.startswith('lds_edge'):
        n, sizes, frames = 20000, (int(name.split('-')[1]),), 2
    elif name == 'two_samples':
        n, sizes, frames = 8000, (1500, 900), 3
    elif name == 'singletons':
        n, sizes, frames = 4096, (4096,), 2
    elif name == 'far':
        n, sizes, frames, spread = 6000, (12,), 3, 50.0
    elif name == 'dyadic_kinks':
        return _dyadic_case(rs)
    elif name == 'one_row':
        n, sizes, frames = 50, (5,), 2
    else:
        assert name == 'random', name
        n, sizes, frames = 6000, (40,), 5
    samples = len(sizes)
    sample = np.sort(rs.randint(0, samples, n)).astype(np.int64)
    tidx = np.stack((sample, rs.randint(0, frames, n)), 1).astype(np.int64)
    lab = np.zeros(n, np.int64)
    for b, k in enumerate(sizes):
        idx = np.nonzero(sample == b)[0]
        lab[idx] = rs.randint(0, k, idx.size)
        if name == 'singletons':
            lab[idx] = rs.permutation(k)
    pts = (rs.randn(n, 3) * spread).astype(np.float32)
    if name == 'far':
        pts += (rs.choice((-2000.0, 2000.0), (n, 3))).astype(np.float32)
    base = np.cumsum((0,) + sizes[:-1]).astype(np.int64)
    ego, motion = _rigid(rs, (samples, frames), 1.0), _rigid(rs, (sum(sizes), frames), 0.5)
    if name == 'far':                                                            # keep the far points far: small rotations would do, identity is plainer
        ego[..., :3, :3] = np.eye(3)
    m = 1 if name == 'one_row' else n // 2
    rows = np.sort(rs.choice(n, m, replace=False)).astype(np.int64)
    tp = (pts + rs.randn(n, 3) * 0.5).astype(np.float32)
    est = np.zeros((n, 2), np.float32)
    case = dict(points=pts, time_indice=tidx, inst_labels=lab, label_base=base, sizes=sizes, ego=ego, inst_motion=motion, transformed_points=tp,
                offset_est=est, rows=rows, kind=kind)
    # estimates a clear distance (>= 0.05 m per coordinate) from the ground truth: the sign of gt - est is decided alike in float32 and float64.  Among
    # the far points the distance grows with the coordinates: an estimate within 2 m of a 2000 m offset is parallel to it to 1e-3, and the gradient of
    # the direction term, the component of gt / |gt| across est, would then be what is left of a thousandfold cancellation
    gt = offset_loss64(**_ref_args(case))['offset_gt']
    est[rows] = (gt + rs.choice((-1.0, 1.0), gt.shape) * rs.uniform(0.05, 2.0, gt.shape) * (1000.0 if name == 'far' else 1.0)).astype(np.float32)
    est[np.setdiff1d(np.arange(n), rows)] = rs.randn(n - m, 2)
    return _freeze_case(case)


def _dyadic_case(rs):
    """1024 points, 64 instances of 16 points, 2 samples of 32 instances, 2 frames.  Coordinates are multiples of 2^-6 below 64, poses the identity or a
    translation by multiples of 2^-4, so every reconstructed point, every 16-point sum and every centre is exact in float32 and float64 alike;
    transformed_points = centre + a multiple of 2^-4, so offset_gt is that multiple, exactly, on both sides."""
    n, k, frames = 1024, 64, 2
    lab_all = rs.permutation(np.repeat(np.arange(k), n // k))
    sample = (lab_all >= 32).astype(np.int64)
    perm = np.argsort(sample, kind='stable')
    lab_all, sample = lab_all[perm], sample[perm]
    tidx = np.stack((sample, rs.randint(0, frames, n)), 1).astype(np.int64)
    lab = lab_all - 32 * sample
    pts = (rs.randint(-64 * 64, 64 * 64, (n, 3)) / 64.0).astype(np.float32)
    ego = np.tile(np.eye(4, dtype=np.float32), (2, frames, 1, 1))
    ego[:, 1, :3, 3] = rs.randint(-64, 65, (2, 3)) / 16.0
    motion = np.tile(np.eye(4, dtype=np.float32), (k, frames, 1, 1))
    motion[::2, :, :3, 3] = rs.randint(-64, 65, (k // 2, frames, 3)) / 16.0
    base = np.array([0, 32], np.int64)
    rows = np.sort(rs.choice(n, 768, replace=False)).astype(np.int64)
    tp = np.zeros((n, 3), np.float32)
    est = (rs.randint(1, 65, (n, 2)) * rs.choice((-1, 1), (n, 2)) / 16.0).astype(np.float32)
    case = dict(points=pts, time_indice=tidx, inst_labels=lab, label_base=base, sizes=(32, 32), ego=ego, inst_motion=motion, transformed_points=tp,
                offset_est=est, rows=rows, kind=None)
    centre_all = np.zeros((n, 2))
    centre_all[rows] = offset_loss64(**_ref_args(case))['offset_gt']             # tp = 0: offset_gt = centre
    kind = np.full(n, 3, np.int64)
    kind[rows] = rs.permutation(np.repeat((0, 1, 2, 3), (192, 192, 96, 288)))
    off = rs.randint(1, 65, (n, 2)) * rs.choice((-1, 1), (n, 2)) / 16.0          # the ground-truth offsets: non-zero multiples of 2^-4
    off[kind == 2] = 0.0
    tp[:, :2] = np.where(np.isin(np.arange(n), rows)[:, None], centre_all - off, 0.0)
    est[kind == 0] = off[kind == 0]
    est[kind == 1] = 0.0
    ordinary = kind == 3
    est[ordinary] = np.where(est[ordinary] == off[ordinary], est[ordinary] + 0.5, est[ordinary])   # ordinary rows stay off the kink, by >= 2^-4
    case['kind'] = kind
    return _freeze_case(case)


def _freeze_case(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _ref_args(case):
    return {k: case[k] for k in ('points', 'time_indice', 'inst_labels', 'label_base', 'ego', 'inst_motion', 'transformed_points', 'offset_est', 'rows')}


def offset_ref(case):
    return offset_loss64(**_ref_args(case))
