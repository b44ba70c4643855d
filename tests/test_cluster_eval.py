"""Instance-segmentation evaluation of the test loop (include/pcacc.h C2; pcaccumulation_amd/cluster_eval.py; FuseLoss.evaluate_cluster).

Golden vectors: tests/golden/cluster_eval.npz -- the reference's toolbox/cluster_eval.py:ClusterEvaluation run on the CPU on constructed scenes
(tests/golden/make_golden_cluster_eval.py): inputs, every accumulator after the calls, the text final_eval wrote.
CPU leg: a numpy restatement of the evaluation written here from its rules reproduces those accumulators exactly (that pins the checker to
the reference); the module's table -> accumulators -> text path, fed with the restatement's tables, reproduces accumulators and text.
GPU leg: pcacc_cluster_eval through FuseLoss.evaluate_cluster on the fixture (== on every list, same text), against the restatement at
4 x 800 k points, run-to-run identical, degenerate inputs, and on the tiny test-mode model's own output."""
import os

import numpy as np
import pytest
import torch

from pcaccumulation_amd import cluster_eval, native
from pcaccumulation_amd.cluster_eval import ClusterEvaluation
from pcaccumulation_amd.config import default_config
from pcaccumulation_amd.loss import FuseLoss

THRESHOLDS = [0.5, 0.6, 0.7, 0.8, 0.9]
FIELDS = ('sample', 'id', 'count', 'cls', 'best')


# ------------------------------------------------------------------------------------------------ the restatement
def restate_tables(est, gt, mos, batch):
    """The rules of the evaluation in numpy.  Per (sample, non-zero id) and side: count, class = 1 iff 2 * moving > count; per pair of equal class in
    a sample: IoU = fp32(inter) / fp32(count_e + count_g - inter); best = max over the other side (0.0 when nothing overlaps; -1.0 for an estimated
    instance whose class has no ground-truth instance in the sample).  -> two dicts of arrays sorted by (sample, id)."""
    batch = batch.astype(np.int64)
    moving = (mos != 0)

    def side(ids):
        uniq, rank = np.unique(ids, return_inverse=True)                  # ascending ids: rank keeps their order
        keep = ids != 0
        key, inv, count = np.unique(batch[keep] * len(uniq) + rank[keep], return_inverse=True, return_counts=True)
        ones = np.bincount(inv, weights=moving[keep], minlength=len(key)).astype(np.int64)
        row = np.full(len(ids), -1, np.int64)
        row[keep] = inv
        return {'sample': key // len(uniq), 'id': uniq[key % len(uniq)], 'count': count.astype(np.int64), 'cls': (2 * ones > count).astype(np.int64)}, row

    e, erow = side(est)
    g, grow = side(gt)
    ne, ng = len(e['id']), len(g['id'])
    has_gt = np.zeros((int(batch.max()) + 1 if len(batch) else 1, 2), bool)
    has_gt[g['sample'], g['cls']] = True
    e['best'] = np.where(has_gt[e['sample'], e['cls']], 0.0, -1.0).astype(np.float32) if ne else np.zeros(0, np.float32)
    g['best'] = np.zeros(ng, np.float32)
    both = (erow >= 0) & (grow >= 0)
    if both.any():
        pair, inter = np.unique(erow[both] * ng + grow[both], return_counts=True)
        pe, pg = pair // ng, pair % ng
        same = e['cls'][pe] == g['cls'][pg]
        pe, pg, inter = pe[same], pg[same], inter[same]
        iou = inter.astype(np.float32) / (e['count'][pe] + g['count'][pg] - inter).astype(np.float32)
        np.maximum.at(e['best'], pe, iou)
        np.maximum.at(g['best'], pg, iou)
    return e, g


def restate_accumulators(e, g, n_batches):
    """The accumulators after one forward() per sample: per sample and class, mean and point-weighted mean of the ground-truth instances' best IoU
    (only when the class has instances), the count of ground-truth instances, and a 1 in tp or fp per estimated instance and threshold -- sums in
    Python doubles, instance by instance in ascending id order."""
    acc = {'cov': [[], []], 'wcov': [[], []], 'total': np.zeros(2), 'tp': {t: [[], []] for t in THRESHOLDS}, 'fp': {t: [[], []] for t in THRESHOLDS}}
    for b in range(n_batches):
        for c in range(2):
            sel = (g['sample'] == b) & (g['cls'] == c)
            best, count = [float(v) for v in g['best'][sel]], [int(v) for v in g['count'][sel]]
            if best:
                s = w = 0
                for v, k in zip(best, count):
                    s += v
                    w += v * k
                acc['cov'][c].append(s / len(best))
                acc['wcov'][c].append(w / sum(count))
            acc['total'][c] += len(best)
            for v in e['best'][(e['sample'] == b) & (e['cls'] == c)]:
                for t in THRESHOLDS:
                    hit = float(v) > t
                    acc['tp'][t][c].append(1.0 if hit else 0.0)
                    acc['fp'][t][c].append(0.0 if hit else 1.0)
    return acc


def _assert_fixture(g, prefix, cov, wcov, total, tp, fp):
    for c in range(2):
        assert list(cov[c]) == list(g[prefix + 'all_mean_cov_%d' % c])
        assert list(wcov[c]) == list(g[prefix + 'all_mean_weighted_cov_%d' % c])
        for t in THRESHOLDS:
            assert list(tp(t)[c]) == list(g[prefix + 'tps_%s_%d' % (t, c)])
            assert list(fp(t)[c]) == list(g[prefix + 'fps_%s_%d' % (t, c)])
    assert list(total) == list(g[prefix + 'total_gt_inst'])


def _assert_state(g, prefix, ev):
    _assert_fixture(g, prefix, ev.all_mean_cov, ev.all_mean_weighted_cov, ev.total_gt_inst, lambda t: ev.tpsins['@%s' % t], lambda t: ev.fpsins['@%s' % t])
    assert ''.join(line + '\n' for line in cluster_eval.final_lines(ev)[1]) == str(g[prefix + 'text'])


def _inputs(g, prefix):
    return g[prefix + 'inst_est'], g[prefix + 'inst_gt'], g[prefix + 'mos'], g[prefix + 'batch']


def _as_rows(t):
    rows = np.zeros(len(t['id']), cluster_eval.ROW_DTYPE)
    for k in FIELDS:
        rows[k] = t[k]
    return rows


# ------------------------------------------------------------------------------------------------ CPU leg
@pytest.mark.parametrize('prefix', ['', 'nan_'])
def test_restatement_reproduces_reference(golden, prefix):
    g = golden('cluster_eval')
    est, gt, mos, batch = _inputs(g, prefix)
    e, gg = restate_tables(est, gt, mos, batch)
    acc = restate_accumulators(e, gg, int(batch.max()) + 1)
    _assert_fixture(g, prefix, acc['cov'], acc['wcov'], acc['total'], lambda t: acc['tp'][t], lambda t: acc['fp'][t])
    if not prefix:                                                        # the constructed cases are really in the fixture
        assert int(batch.max()) + 1 >= 3 and gt.max() > 2 ** 53
        best0 = set(e['best'][e['sample'] == 0].tolist())
        for p, q in ((1, 2), (3, 5), (7, 10), (4, 5), (9, 10)):
            assert float(np.float32(p) / np.float32(q)) in best0
        assert -1.0 in e['best'] and 0.0 in gg['best']


def test_threshold_comparisons_of_exact_ratios():
    """`ovmax > threshold` compares the fp32 IoU widened to double with a double constant: 3/5 and 4/5 pass their own threshold, 1/2, 7/10 and 9/10 do not."""
    f = lambda p, q: float(np.float32(p) / np.float32(q))
    assert f(3, 5) > 0.6 and f(4, 5) > 0.8
    assert not f(7, 10) > 0.7 and not f(9, 10) > 0.9 and not f(1, 2) > 0.5


@pytest.mark.parametrize('prefix', ['', 'nan_'])
def test_module_tables_to_accumulators_to_text(golden, prefix, tmp_path):
    g = golden('cluster_eval')
    est, gt, mos, batch = _inputs(g, prefix)
    e, gg = restate_tables(est, gt, mos, batch)
    ev = ClusterEvaluation({'save_dir': str(tmp_path)})
    assert os.listdir(str(tmp_path)) == []                                # the constructor opens nothing
    cluster_eval.accumulate(ev, _as_rows(e), _as_rows(gg), int(batch.max()) + 1)
    _assert_state(g, prefix, ev)
    assert ev.num_classes == 2 and ev.iou_threshold == THRESHOLDS and sorted(ev.tpsins) == ['@%s' % t for t in THRESHOLDS]
    res = ev.final_eval()
    ev.final_eval()                                                       # appended, as the reference's 'a' mode does
    assert open(os.path.join(str(tmp_path), 'cluster_eval.txt')).read() == 2 * str(g[prefix + 'text'])
    assert res['MUCov'].dtype == np.float64 and set(res['precision']) == set('@%s' % t for t in THRESHOLDS)
    if prefix:
        assert np.isnan(res['MUCov'][0]) and np.isnan(res['precision']['@0.5'][0]) and res['recall']['@0.5'][1] == 1.0


def test_parse_tables_orders_rows_and_reports_status():
    cap = 4
    buf = np.zeros(native.CLUSTER_EVAL_HEADER_BYTES + 2 * cap * native.CLUSTER_EVAL_ROW_BYTES, np.uint8)
    rows = buf[native.CLUSTER_EVAL_HEADER_BYTES:].view(cluster_eval.ROW_DTYPE)
    for k, (s, i) in enumerate([(1, 5), (0, 2 ** 40), (0, -3)]):
        rows[k]['sample'], rows[k]['id'] = s, i
    rows[cap]['id'] = 9
    buf[:16].view(np.int32)[:] = [0, 3, 1, 0]
    status, e, g = cluster_eval.parse_tables(buf, cap)
    assert status == 0 and [(int(r['sample']), int(r['id'])) for r in e] == [(0, -3), (0, 2 ** 40), (1, 5)] and len(g) == 1 and g[0]['id'] == 9
    buf[:4].view(np.int32)[0] = cluster_eval.ST_INST
    assert cluster_eval.parse_tables(buf, cap)[0] == cluster_eval.ST_INST


def test_fuse_loss_creates_no_file_and_no_state(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = dict(default_config('waymo', 'test', n_sweeps=3, xy_range=8)['loss'])
    cfg['save_dir'] = str(tmp_path)
    loss = FuseLoss(cfg)
    assert '_cluster_eval_offset' not in loss.__dict__ and [n for n, _ in loss.named_modules() if 'cluster' in n] == []
    ev = loss.cluster_eval_offset
    assert isinstance(ev, ClusterEvaluation) and loss.cluster_eval_offset is ev and ev.save_dir == str(tmp_path)
    assert [n for n, _ in loss.named_modules() if 'cluster' in n] == [] and os.listdir(str(tmp_path)) == []


def test_evaluate_cluster_refuses_cpu_tensors():
    loss = FuseLoss(default_config('waymo', 'test', n_sweeps=3, xy_range=8)['loss'])
    z = torch.zeros(8, 1, dtype=torch.int64)
    before = cluster_eval.transfers
    with pytest.raises(native.NativeError):
        loss.evaluate_cluster({'inst_labels_est': torch.ones(8, dtype=torch.int64), '_n_batches': 1},
                              {'time_indice': torch.zeros(8, 2, dtype=torch.float64), 'inst_labels': z + 1, 'sd_labels': z})
    with pytest.raises(native.NativeError):
        ClusterEvaluation()(z[:, 0], z[:, 0], z[:, 0].float())
    assert cluster_eval.transfers == before


def test_entry_points_are_declared_and_exported():
    assert 'pcacc_cluster_eval' in native.EXPORTS and 'pcacc_cluster_eval_workspace_bytes' in native.EXPORTS
    assert native.EXPORTS.index('pcacc_cluster_eval') > native.EXPORTS.index('pcacc_cluster')              # the section after C1


# ------------------------------------------------------------------------------------------------ GPU leg
DEV = 'cuda:0'


def _dict_inputs(est, gt, mos, batch, with_n_batches=True):
    dev = torch.device(DEV)
    n = len(est)
    ti = np.stack([batch.astype(np.float64), np.zeros(n)], 1)                 # collate_fn's layout: (sample, frame) as float64
    pred = {'inst_labels_est': torch.from_numpy(est).to(dev)}
    if with_n_batches:
        pred['_n_batches'] = int(batch.max()) + 1
    inp = {'time_indice': torch.from_numpy(ti).to(dev), 'inst_labels': torch.from_numpy(gt).to(dev)[:, None],
           'sd_labels': torch.from_numpy(mos).to(dev)[:, None]}
    return pred, inp


def _gpu_tables(est, gt, mos, batch, n_batches, **kw):
    dev = torch.device(DEV)
    t = lambda a: a.to(dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return cluster_eval.instance_tables(t(est), t(gt), t(mos), t(batch).to(torch.int32), n_batches, **kw)


def _assert_tables(got, want):
    assert len(got) == len(want['id'])
    for k in FIELDS:
        assert np.array_equal(got[k].astype(want[k].dtype), want[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('prefix', ['', 'nan_'])
def test_evaluate_cluster_fixture_gpu(golden, prefix):
    g = golden('cluster_eval')
    est, gt, mos, batch = _inputs(g, prefix)
    for with_n in (True, False):
        loss = FuseLoss(default_config('waymo', 'test', n_sweeps=3, xy_range=8)['loss'])
        before = cluster_eval.transfers
        loss.evaluate_cluster(*_dict_inputs(est, gt, mos, batch, with_n))
        assert cluster_eval.transfers == before + 1
        _assert_state(g, prefix, loss.cluster_eval_offset)
    # the reference's per-sample forward(), with the float labels libs/loss.py:265 passes
    ev = ClusterEvaluation()
    dev = torch.device(DEV)
    for b in range(int(batch.max()) + 1):
        sel = batch == b
        ev(torch.from_numpy(est[sel]).to(dev), torch.from_numpy(gt[sel]).to(dev), torch.from_numpy(mos[sel]).to(dev).float())
    _assert_state(g, prefix, ev)


def _scale_scene(seed, n_batches, n_per, n_inst, tiny):
    """n_batches x n_per points.  tiny: n_inst instances of a handful of points per sample and side; else n_inst ground-truth instances per sample and
    an estimate that follows them with noise (shifted borders, relabelled and dropped points).  Ids large and sparse on the ground-truth side."""
    rng = np.random.RandomState(seed)
    n = n_batches * n_per
    batch = np.repeat(np.arange(n_batches, dtype=np.int32), n_per)
    ids = rng.permutation(np.unique(rng.randint(1, 2 ** 40, 2 * n_inst))[:n_inst].astype(np.int64)) * 4099 + 1
    if tiny:
        slot = rng.randint(0, 40 * n_inst, n)
        gt = np.where(slot < n_inst, ids[slot % n_inst], 0)
        slot_e = np.where(rng.rand(n) < 0.7, slot, rng.randint(0, 40 * n_inst, n))
        est = np.where(slot_e < n_inst, slot_e + 1, 0).astype(np.int64)
    else:
        pos = rng.rand(n) * n_inst * 3                                        # a third of the line is covered by instances
        k = np.floor(pos).astype(np.int64)
        gt = np.where(k % 3 == 0, ids[k // 3], 0)
        ke = np.floor(pos + rng.randn(n) * 0.08).astype(np.int64) % (3 * n_inst)
        est = np.where(ke % 3 == 0, ke // 3 + 1, 0)
        est = np.where(rng.rand(n) < 0.05, rng.randint(0, n_inst + 1, n), est).astype(np.int64)
    mos = ((gt % 2 == 1) ^ (rng.rand(n) < 0.1)).astype(np.int64)
    return est, gt.astype(np.int64), mos, batch


@pytest.mark.gpu
@pytest.mark.parametrize('tiny,n_inst', [(False, 300), (True, 6000)])
def test_tables_at_scale_gpu(tiny, n_inst):
    est, gt, mos, batch = _scale_scene(3 + tiny, 4, 800000, n_inst, tiny)
    want_e, want_g = restate_tables(est, gt, mos, batch)
    assert len(want_g['id']) >= (4 * n_inst * 9) // 10
    before = cluster_eval.transfers
    got_e, got_g, cap = _gpu_tables(est, gt, mos, batch, 4)
    if tiny:                                                                  # many thousands of tiny instances: the default tables are too small and grow
        assert len(want_e['id']) > 4096 and cap >= len(want_e['id']) and cluster_eval.transfers > before + 1
        assert np.median(want_g['count']) <= 8
    else:
        assert cluster_eval.transfers == before + 1
    _assert_tables(got_e, want_e)
    _assert_tables(got_g, want_g)
    assert (got_e['best'] > 0.5).any() and (got_e['cls'] == 0).any() and (got_e['cls'] == 1).any()
    # run-to-run identical, every byte of every row
    again_e, again_g, _ = _gpu_tables(est, gt, mos, batch, 4, inst_capacity=cap)
    assert got_e.tobytes() == again_e.tobytes() and got_g.tobytes() == again_g.tobytes()
    # explicit small pair table: grows instead of truncating
    few_e, few_g, _ = _gpu_tables(est, gt, mos, batch, 4, inst_capacity=cap, pair_capacity=64)
    assert got_e.tobytes() == few_e.tobytes() and got_g.tobytes() == few_g.tobytes()


@pytest.mark.gpu
def test_degenerate_inputs_gpu():
    z = np.zeros(0, np.int64)
    e, g, _ = _gpu_tables(z, z, z, z.astype(np.int32), 1)
    assert len(e) == 0 and len(g) == 0
    ev = ClusterEvaluation()
    ev(torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV))
    assert ev.all_mean_cov == [[], []] and list(ev.total_gt_inst) == [0.0, 0.0]

    rng = np.random.RandomState(0)
    n = 5000
    batch = np.repeat(np.arange(2, dtype=np.int32), n // 2)
    mos = (rng.rand(n) < 0.5).astype(np.int64)
    some = rng.randint(0, 4, n).astype(np.int64)
    zero = np.zeros(n, np.int64)
    for est, gt in ((zero, zero), (some, zero), (zero, some), (zero + 7, some), (zero + 7, zero + 7)):       # background on one / both sides; one instance = the sample
        want_e, want_g = restate_tables(est, gt, mos, batch)
        got_e, got_g, _ = _gpu_tables(est, gt, mos, batch, 2)
        _assert_tables(got_e, want_e)
        _assert_tables(got_g, want_g)
    # ids near 2^62, negative ids (instances like any other, as torch.unique treats them), ids that differ in the high word only
    pool = np.array([0, -1, -2 ** 62, 2 ** 62 - 1, 2 ** 62 - 2, 1, 1 + 2 ** 32, 2 ** 61, -5], np.int64)
    est, gt = pool[rng.randint(0, len(pool), n)], pool[rng.randint(0, len(pool), n)]
    gt[:400] = est[:400]
    want_e, want_g = restate_tables(est, gt, mos, batch)
    got_e, got_g, _ = _gpu_tables(est, gt, mos, batch, 2)
    _assert_tables(got_e, want_e)
    _assert_tables(got_g, want_g)
    assert int(got_e['id'].min()) == -2 ** 62 and (got_e['id'] == -1).any()
    # the label types a caller may hold: the same tables from int64, float32 and bool
    for m in (torch.from_numpy(mos).float(), torch.from_numpy(mos).bool()):
        e2, g2, _ = _gpu_tables(est, gt, m, batch, 2)
        assert e2.tobytes() == got_e.tobytes() and g2.tobytes() == got_g.tobytes()
    # a sample index outside the batch is an error, not a silent drop
    with pytest.raises(native.NativeError):
        _gpu_tables(est, gt, mos, batch, 1)


@pytest.mark.gpu
def test_sample_above_2_24_points_is_an_error_gpu():
    """round(fp32 mean) is the integer rule only while fp32 sums of 0/1 are exact: more than 2^24 points in a sample raise."""
    dev = torch.device(DEV)
    n = 2 ** 24 + 1
    ids = torch.ones(n, dtype=torch.int64, device=dev)
    batch = torch.zeros(n, dtype=torch.int32, device=dev)
    batch[-5:] = 1
    e, g, _ = cluster_eval.instance_tables(ids, ids, ids, batch, 2)          # 2^24 - 4 and 5 points: fine
    assert [int(c) for c in e['count']] == [n - 5, 5] and [float(b) for b in g['best']] == [1.0, 1.0]
    with pytest.raises(native.NativeError, match='2\\^24'):
        cluster_eval.instance_tables(ids, ids, ids, torch.zeros(n, dtype=torch.int32, device=dev), 2)       # known on the device only
    with pytest.raises(native.NativeError):
        cluster_eval.instance_tables(ids, ids, ids, batch, 1)                  # known from the sizes


@pytest.mark.gpu
def test_end_to_end_tiny_model_gpu(golden, monkeypatch):
    """The tiny test-mode model of test_cluster.py: evaluate_cluster on its own output equals the restatement on out['inst_labels_est']; the
    forward itself makes no transfer through this module, and the evaluation is ONE Tensor.cpu() with no .item() / .tolist() beside it."""
    from helpers import make_batch
    from pcaccumulation_amd.motionnet import MotionNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    dev = torch.device(DEV)
    g = golden('model_tiny_test')
    cfg = default_config('waymo', 'test', n_sweeps=3, xy_range=8)
    inp = make_batch(cfg, [int(s) for s in g['seeds']], int(g['n_frames']), int(g['pts_per_frame']))
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in zip(g['tweak_keys'], g['tweak_vals']):
            sd[str(k)] += torch.from_numpy(v)
        sd['motionhead.offset_head.seg_head.3.weight'] *= float(g['offset_scale'])
        sd['motionhead.offset_head.seg_head.3.bias'] *= float(g['offset_scale'])
        sd['motionhead.mos_seg.seg_head.3.bias'] += torch.tensor([0.0, float(g['mos_shift'])])
    model = model.to(dev).eval().channels_last_()
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    torch.manual_seed(int(g['fwd_seed']))
    before = cluster_eval.transfers
    with torch.no_grad():
        out = model(inp)
    assert cluster_eval.transfers == before                                   # the forward pass does not know this module
    calls = {'cpu': 0, 'other': 0}
    real_cpu, real_item, real_tolist = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (calls.__setitem__('cpu', calls['cpu'] + 1), real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, 'item', lambda self: (calls.__setitem__('other', calls['other'] + 1), real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, 'tolist', lambda self: (calls.__setitem__('other', calls['other'] + 1), real_tolist(self))[1])
    loss = FuseLoss(cfg['loss'])
    loss.evaluate_cluster(out, inp)
    monkeypatch.undo()
    assert cluster_eval.transfers == before + 1 and calls == {'cpu': 1, 'other': 0}
    est = out['inst_labels_est'].cpu().numpy()
    assert est.max() > 0
    batch = inp['time_indice'][:, 0].cpu().numpy().astype(np.int32)
    e, gg = restate_tables(est, inp['inst_labels'][:, 0].cpu().numpy(), inp['sd_labels'][:, 0].cpu().numpy(), batch)
    acc = restate_accumulators(e, gg, int(batch.max()) + 1)
    ev = loss.cluster_eval_offset
    assert [list(v) for v in ev.all_mean_cov] == acc['cov'] and [list(v) for v in ev.all_mean_weighted_cov] == acc['wcov']
    assert list(ev.total_gt_inst) == list(acc['total']) and sum(acc['total']) > 0
    for t in THRESHOLDS:
        assert ev.tpsins['@%s' % t] == acc['tp'][t] and ev.fpsins['@%s' % t] == acc['fp'][t]
    loss.evaluate_cluster(out, inp)                                           # a second batch appends
    assert cluster_eval.transfers == before + 2 and [len(v) for v in ev.all_mean_cov] == [2 * len(v) for v in acc['cov']]
