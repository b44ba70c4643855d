"""Instance-segmentation evaluation of the test loop: host mirror of toolbox/cluster_eval.py (ClusterEvaluation) over the HIP path of
include/pcacc.h C2.

The reference compares every estimated instance of a sample with every ground-truth instance through boolean masks of length N and reads two
sums per pair back to the host (cluster_eval.py:104-114, 134-142).  Here one call builds, for the whole batch, a table row per (sample,
estimated instance) and per (sample, ground-truth instance) -- id, point count, class, best IoU, all integers or one fp32 division, so they are
the reference's numbers bit for bit (csrc/cluster_eval.hip) -- and ONE device -> host transfer brings both tables over.  What is left is the
reference's own small sequential arithmetic in Python doubles, in the reference's order (`accumulate`, testable without a GPU), on the
reference's accumulators under the reference's names."""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import native

# one table row as csrc/cluster_eval.hip (CeRow) lays it out
ROW_DTYPE = np.dtype([('id', '<i8'), ('count', '<u4'), ('moving', '<u4'), ('sample', '<i4'), ('cls', '<i4'), ('best', '<f4'), ('pad', '<i4')])
assert ROW_DTYPE.itemsize == native.CLUSTER_EVAL_ROW_BYTES

ST_INST, ST_PAIR, ST_SAMPLE, ST_BATCH = 1, 2, 4, 8

# device -> host transfers made by this module since import (tests: exactly one per evaluated batch unless a table had to grow)
transfers = 0


def _sorted(rows):
    """Rows in the order the reference visits instances: sample by sample (libs/loss.py:268), ascending id inside one (torch.unique)."""
    return rows[np.lexsort((rows['id'], rows['sample']))]


def parse_tables(buf, inst_capacity):
    """The bytes pcacc_cluster_eval wrote (host copy, uint8) -> (status, estimated rows, ground-truth rows), rows sorted by (sample, id)."""
    head = buf[:native.CLUSTER_EVAL_HEADER_BYTES].view(np.int32)
    status, n_est, n_gt = int(head[0]), int(head[1]), int(head[2])
    if status:
        return status, None, None
    rows = buf[native.CLUSTER_EVAL_HEADER_BYTES:].view(ROW_DTYPE)
    return 0, _sorted(rows[:n_est]), _sorted(rows[inst_capacity:inst_capacity + n_gt])


MIN_PAIR_CAPACITY = 1 << 20


def _tables(inst_est, inst_gt, mos, batch, n_batches, inst_capacity, pair_capacity):
    """instance_tables, also returning the pair capacity that was enough."""
    global transfers
    n = int(inst_est.shape[0])
    inst_capacity = int(inst_capacity)
    while True:
        # an estimate that overlaps every ground-truth instance a little makes E * G pairs from few instances: the pair table is sized for that from the start
        pairs = int(pair_capacity) if pair_capacity else min(n + 1, max(4 * inst_capacity, MIN_PAIR_CAPACITY))
        out = native.cluster_eval(inst_est, inst_gt, mos, batch, n_batches, inst_capacity, pairs)
        buf = out.cpu().numpy()
        transfers += 1
        status, est, gt = parse_tables(buf, inst_capacity)
        if status == 0:
            return est, gt, inst_capacity, pairs
        if status & ST_BATCH:
            raise native.NativeError('cluster_eval: a batch index lies outside [0, %d)' % n_batches)
        if status & ST_SAMPLE:
            raise native.NativeError('cluster_eval: a sample has more than 2^24 points; the class of an instance (round of an fp32 mean of its '
                                     '0/1 labels, toolbox/cluster_eval.py:85) is not an exact quantity there and is not guessed')
        grown_inst, grown_pairs = min(4 * inst_capacity, n + 1), min(4 * pairs, n + 1)
        if (status & ST_INST and grown_inst <= inst_capacity) or (status & ST_PAIR and grown_pairs <= pairs):
            raise native.NativeError('cluster_eval: tables of %d rows / %d pairs overflowed on %d points' % (inst_capacity, pairs, n))
        if status & ST_INST:
            inst_capacity = grown_inst
        pair_capacity = grown_pairs if status & ST_PAIR else pair_capacity


def instance_tables(inst_est, inst_gt, mos, batch, n_batches, inst_capacity=4096, pair_capacity=None):
    """-> (estimated rows, ground-truth rows, inst_capacity used): numpy arrays of ROW_DTYPE sorted by (sample, id).  One kernel call and one
    transfer.  pair_capacity None: room for 2^20 non-empty pairs (never more than n + 1).  When the batch holds more instances or non-empty
    pairs than the tables were sized for, the call is repeated with four times the room (n points make at most n rows and n pairs, so the
    growth ends): a small table never truncates."""
    return _tables(inst_est, inst_gt, mos, batch, n_batches, inst_capacity, pair_capacity)[:3]


def accumulate(state, est_rows, gt_rows, n_batches):
    """toolbox/cluster_eval.py:98-152 for samples 0 .. n_batches - 1 from their table rows (fields sample, id, count, cls, best; sorted by
    (sample, id)): appends to the accumulators of `state` (a ClusterEvaluation, or anything with its attributes) exactly what the
    reference's forward() appends sample by sample -- Python doubles, same operations, same order."""
    thresholds = state.iou_threshold
    for b in range(n_batches):
        est_b, gt_b = est_rows[est_rows['sample'] == b], gt_rows[gt_rows['sample'] == b]
        for sem_idx in range(state.num_classes):                      # :98-124 coverage
            sum_cov, mean_weighted_cov, num_gt_point = 0, 0, 0
            rows = gt_b[gt_b['cls'] == sem_idx]
            for r in rows:
                ovmax = float(r['best'])                              # fp32 widened, as float(tensor) does at :111
                num_inst_gt_point = int(r['count'])
                num_gt_point += num_inst_gt_point
                sum_cov += ovmax
                mean_weighted_cov += ovmax * num_inst_gt_point
            n_inst = len(rows)
            if n_inst:
                state.all_mean_cov[sem_idx].append(sum_cov / n_inst)
                mean_weighted_cov /= num_gt_point
                state.all_mean_weighted_cov[sem_idx].append(mean_weighted_cov)
        for sem_idx in range(state.num_classes):                      # :127-152 precision / recall
            rows = est_b[est_b['cls'] == sem_idx]
            tp = {'@%s' % t: [0.] * len(rows) for t in thresholds}
            fp = {'@%s' % t: [0.] * len(rows) for t in thresholds}
            state.total_gt_inst[sem_idx] += int((gt_b['cls'] == sem_idx).sum())
            for idx, r in enumerate(rows):
                ovmax = float(r['best'])
                for t in thresholds:
                    if ovmax > t:
                        tp['@%s' % t][idx] = 1
                    else:
                        fp['@%s' % t][idx] = 1
            for t in thresholds:
                state.tpsins['@%s' % t][sem_idx] += tp['@%s' % t]
                state.fpsins['@%s' % t][sem_idx] += fp['@%s' % t]


def final_lines(state):
    """toolbox/cluster_eval.py:33-68: -> (results, the lines final_eval logs).  float64 stands where the reference says np.float; an empty
    class gives nan exactly where the reference prints nan."""
    k = state.num_classes
    mucov, mwcov = np.zeros(k), np.zeros(k)
    precision, recall = np.zeros(k), np.zeros(k)
    results = {}
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        for sem_idx in range(k):
            mucov[sem_idx] = np.mean(state.all_mean_cov[sem_idx])
            mwcov[sem_idx] = np.mean(state.all_mean_weighted_cov[sem_idx])
        lines = ['Instance Segmentation MUCov: {}'.format(mucov), 'Instance Segmentation mMUCov: {}'.format(np.mean(mucov)),
                 'Instance Segmentation MWCov: {}'.format(mwcov), 'Instance Segmentation mMWCov: {}'.format(np.mean(mwcov))]
        results.update(MUCov=mucov.copy(), mMUCov=np.mean(mucov), MWCov=mwcov.copy(), mMWCov=np.mean(mwcov), precision={}, recall={})
        for threshold in state.iou_threshold:
            for sem_idx in range(k):
                tp = np.sum(np.asarray(state.tpsins['@%s' % threshold][sem_idx]).astype(np.float64))
                fp = np.sum(np.asarray(state.fpsins['@%s' % threshold][sem_idx]).astype(np.float64))
                recall[sem_idx] = tp / state.total_gt_inst[sem_idx]
                precision[sem_idx] = tp / (tp + fp)
            lines += ['IoU threshold @%s' % threshold, 'Instance Segmentation Precision: {}'.format(precision),
                      'Instance Segmentation mPrecision: {}'.format(np.mean(precision)), 'Instance Segmentation Recall: {}'.format(recall),
                      'Instance Segmentation mRecall: {}'.format(np.mean(recall))]
            results['precision']['@%s' % threshold], results['recall']['@%s' % threshold] = precision.copy(), recall.copy()
    lines.append('\n')
    return results, lines


class ClusterEvaluation(nn.Module):
    """toolbox/cluster_eval.py:15-152 with the reference's state: num_classes, iou_threshold, all_mean_cov, all_mean_weighted_cov,
    total_gt_inst, tpsins / fpsins keyed '@0.5' ...  forward() takes one sample like the reference's, forward_batch() a whole batch with its
    batch index: one kernel call, one transfer.  cfg['save_dir'] (optional) is where final_eval() appends cluster_eval.txt; the file is
    opened there, never here."""

    def __init__(self, cfg=None):
        super(ClusterEvaluation, self).__init__()
        self.num_classes = 2
        self.iou_threshold = [0.5, 0.6, 0.7, 0.8, 0.9]
        self.all_mean_cov = [[] for _ in range(self.num_classes)]
        self.all_mean_weighted_cov = [[] for _ in range(self.num_classes)]
        self.total_gt_inst = np.zeros(self.num_classes)
        self.tpsins, self.fpsins = dict(), dict()
        for threshold in self.iou_threshold:
            self.tpsins[f'@{threshold}'] = [[] for _ in range(self.num_classes)]
            self.fpsins[f'@{threshold}'] = [[] for _ in range(self.num_classes)]
        self.save_dir = (cfg or {}).get('save_dir')
        self.inst_capacity, self.pair_capacity = 4096, None     # grow with the largest batch seen, so a big scene pays its second call once

    def forward_batch(self, inst_est, inst_gt, mos_label, batch, n_batches):
        """inst_est, inst_gt [N] (0 = background), mos_label [N] (0 static / 1 dynamic; int64, float32 or bool), batch [N] sample index:
        what forward() does for every sample 0 .. n_batches - 1 in turn.  Device tensors only."""
        for name, t in (('inst_est', inst_est), ('inst_gt', inst_gt), ('mos_label', mos_label), ('batch', batch)):
            if not t.is_cuda:
                raise native.NativeError('cluster evaluation: %s must live on the GPU (got %s); the HIP path has no CPU fallback' % (name, t.device))
        if mos_label.dtype not in (torch.int64, torch.float32, torch.bool, torch.uint8):
            mos_label = mos_label.float()
        est, gt, self.inst_capacity, pairs = _tables(inst_est.long().contiguous(), inst_gt.long().contiguous(), mos_label.contiguous(),
                                                     batch.to(torch.int32).contiguous(), int(n_batches), self.inst_capacity, self.pair_capacity)
        if pairs > MIN_PAIR_CAPACITY:
            self.pair_capacity = pairs
        accumulate(self, est, gt, int(n_batches))

    def forward(self, inst_est, inst_gt, mos_label):
        """cluster_eval.py:71-152: one sample."""
        self.forward_batch(inst_est, inst_gt, mos_label, torch.zeros(inst_est.shape[0], dtype=torch.int32, device=inst_est.device), 1)

    def final_eval(self, save_dir=None):
        """cluster_eval.py:33-68: prints the summary, appends it to <save_dir>/cluster_eval.txt when a save_dir is known (argument, or
        cfg['save_dir']), and returns the numbers."""
        results, lines = final_lines(self)
        save_dir = save_dir or self.save_dir
        if save_dir:
            with open(os.path.join(save_dir, 'cluster_eval.txt'), 'a') as f:
                for line in lines:
                    f.write(line + '\n')
        for line in lines:
            print(line)
        return results
