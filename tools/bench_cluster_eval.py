"""Time the instance-segmentation evaluation of the test loop (include/pcacc.h C2, pcaccumulation_amd/cluster_eval.py) at the clustering
benchmark's size, and beside it, on the same device, the plain torch formulation a user would run otherwise: one boolean mask per instance,
every (estimated, ground-truth) pair of a class compared through `(a & b).sum() / (a | b).sum()` read back to the host
(toolbox/cluster_eval.py:98-142 restated).  Each leg is a child process under its own time limit; both times go to
profiles/cluster_eval_bench.txt.  Nothing is gated on them.
Usage: python tools/bench_cluster_eval.py [--batch 4] [--points 800000] [--instances 200] [--iters 20] [--out profiles/cluster_eval_bench.txt]
       (--leg new | torch runs one leg in this process and prints its JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(seed, n_batches, n_per, n_inst):
    """n_inst ground-truth instances per sample (large sparse ids) and an estimate that follows them with shifted borders and 5 % relabelled points;
    two thirds of the points are background.  Points of an instance are spread over the sample, as the frames of a sequence interleave them."""
    rng = np.random.RandomState(seed)
    n = n_batches * n_per
    batch = np.repeat(np.arange(n_batches, dtype=np.int32), n_per)
    ids = rng.permutation(np.unique(rng.randint(1, 2 ** 40, 2 * n_inst))[:n_inst].astype(np.int64)) * 4099 + 1
    pos = rng.rand(n) * n_inst * 3
    k = np.floor(pos).astype(np.int64)
    gt = np.where(k % 3 == 0, ids[k // 3], 0).astype(np.int64)
    ke = np.floor(pos + rng.randn(n) * 0.08).astype(np.int64) % (3 * n_inst)
    est = np.where(ke % 3 == 0, ke // 3 + 1, 0)
    est = np.where(rng.rand(n) < 0.05, rng.randint(0, n_inst + 1, n), est).astype(np.int64)
    mos = ((gt % 2 == 1) ^ (rng.rand(n) < 0.1)).astype(np.int64)
    return est, gt, mos, batch


def leg_new(a, est, gt, mos, batch):
    import torch
    from pcaccumulation_amd import cluster_eval, native
    dev = torch.device('cuda:0')
    t_est, t_gt, t_mos, t_b = (torch.from_numpy(x).to(dev) for x in (est, gt, mos, batch))
    ev = cluster_eval.ClusterEvaluation()
    ev.forward_batch(t_est, t_gt, t_mos, t_b, a.batch)                       # warm-up: code object, table size
    cap, pairs = ev.inst_capacity, ev.pair_capacity or cluster_eval.MIN_PAIR_CAPACITY
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        native.cluster_eval(t_est, t_gt, t_mos, t_b, a.batch, cap, pairs)
    e1.record()
    torch.cuda.synchronize()
    kernels_ms = e0.elapsed_time(e1) / a.iters                               # device events around the launches of one call
    t = time.perf_counter()
    for _ in range(a.iters):
        e_rows, g_rows, _ = cluster_eval.instance_tables(t_est, t_gt, t_mos, t_b, a.batch, cap)      # ends in the transfer: a synchronising copy
    tables_ms = (time.perf_counter() - t) * 1e3 / a.iters
    t = time.perf_counter()
    for _ in range(a.iters):
        cluster_eval.ClusterEvaluation().forward_batch(t_est, t_gt, t_mos, t_b, a.batch)              # + the reference's host sums
    full_ms = (time.perf_counter() - t) * 1e3 / a.iters
    return {'leg': 'new', 'points': int(len(est)), 'est_rows': int(len(e_rows)), 'gt_rows': int(len(g_rows)), 'inst_capacity': int(cap),
            'kernels_ms': round(kernels_ms, 3), 'tables_with_transfer_ms': round(tables_ms, 3), 'evaluate_batch_ms': round(full_ms, 3),
            'best_sum': float(np.sum(e_rows['best'].astype(np.float64)) + np.sum(g_rows['best'].astype(np.float64)))}


def leg_torch(a, est, gt, mos, batch):
    import torch
    dev = torch.device('cuda:0')
    t_est, t_gt, t_b = (torch.from_numpy(x).to(dev) for x in (est, gt, batch))
    t_mos = torch.from_numpy(mos).to(dev).float()

    def masks(ids):
        out = [[], []]
        for u in torch.unique(ids):
            if u != 0:
                m = ids == u
                out[round(t_mos_b[m].mean().item())].append(m)
        return out

    def best(mine, others, start):
        res = []
        for m in mine:
            top = start
            for o in others:
                top = max(top, float((m & o).sum() / (m | o).sum()))
            res.append(top)
        return res
    (t_est[:10] == 1).sum().item()                                           # warm-up of the few kernels involved
    torch.cuda.synchronize()
    t = time.perf_counter()
    total, pairs = 0.0, 0
    for b in range(a.batch):
        sel = t_b == b
        t_mos_b = t_mos[sel]
        e_m, g_m = masks(t_est[sel]), masks(t_gt[sel])
        for c in range(2):
            total += sum(best(g_m[c], e_m[c], 0.)) + sum(best(e_m[c], g_m[c], -1.))
            pairs += 2 * len(g_m[c]) * len(e_m[c])
    torch.cuda.synchronize()
    return {'leg': 'torch', 'points': int(len(est)), 'pairs_compared': pairs, 'evaluate_batch_ms': round((time.perf_counter() - t) * 1e3, 1),
            'best_sum': total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--points', type=int, default=800000)
    ap.add_argument('--instances', type=int, default=200)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--leg', choices=['new', 'torch'])
    ap.add_argument('--limit', type=int, default=400, help='seconds per leg')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cluster_eval_bench.txt'))
    a = ap.parse_args()
    if a.leg:
        est, gt, mos, batch = scene(0, a.batch, a.points, a.instances)
        print(json.dumps((leg_new if a.leg == 'new' else leg_torch)(a, est, gt, mos, batch)))
        return
    lines = []
    for leg in ('new', 'torch'):                                             # a leg that fails or runs out of time ends the run: nothing else is started on the device
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--leg', leg, '--batch', str(a.batch),
               '--points', str(a.points), '--instances', str(a.instances), '--iters', str(a.iters)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if res.returncode != 0:
            sys.exit('leg %s ended with status %d' % (leg, res.returncode))
        lines.append(res.stdout.strip().splitlines()[-1])
        print(lines[-1])
    new, ref = json.loads(lines[0]), json.loads(lines[1])
    same = abs(new['best_sum'] - ref['best_sum']) <= 1e-9 * max(1.0, abs(ref['best_sum']))
    head = ('cluster evaluation, %d samples x %d points, %d instances per sample and side; same device, same tensors\n'
            'new path: kernels %.3f ms (device events), tables with their transfer %.3f ms, whole evaluate_batch %.3f ms (wall, mean of %d)\n'
            'torch pairwise masks: %.1f ms (wall, one pass, %d pairs compared); sums of best IoUs agree: %s\n'
            % (a.batch, a.points, a.instances, new['kernels_ms'], new['tables_with_transfer_ms'], new['evaluate_batch_ms'], a.iters,
               ref['evaluate_batch_ms'], ref['pairs_compared'], same))
    with open(a.out, 'w') as f:
        f.write(head + '\n'.join(lines) + '\n')
    print(head)


if __name__ == '__main__':
    main()
