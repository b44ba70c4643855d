"""Golden vectors for the instance-segmentation evaluation of the test loop: the reference's toolbox/cluster_eval.py:ClusterEvaluation run
here on the CPU, sample by sample as libs/loss.py:267-270 calls it, on constructed scenes.  Stored: the inputs, every accumulator after the
calls, and the text final_eval wrote.  Run: python tests/golden/make_golden_cluster_eval.py"""
import os
import sys
import tempfile
from fractions import Fraction

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

THRESHOLDS = [0.5, 0.6, 0.7, 0.8, 0.9]


class Scene(object):
    """Points of one sample as (est id, gt id, moving) triples, appended block by block."""

    def __init__(self):
        self.est, self.gt, self.mos = [], [], []

    def add(self, n, est, gt, mos):
        """n points with estimated id `est`, ground-truth id `gt`; mos: 0, 1, or the number of moving points among them."""
        m = np.zeros(n, np.int64)
        m[:(n if mos is True else int(mos))] = 1
        self.est.append(np.full(n, est, np.int64))
        self.gt.append(np.full(n, gt, np.int64))
        self.mos.append(m)

    def arrays(self, rng):
        est, gt, mos = np.concatenate(self.est), np.concatenate(self.gt), np.concatenate(self.mos)
        p = rng.permutation(len(est))
        return est[p], gt[p], mos[p]


def exact_scene():
    """IoU exactly 1/2, 3/5, 7/10, 4/5, 9/10 between moving instances; ties of the moving fraction; sparse large ids; a cross-class overlap."""
    s = Scene()
    big = [10 ** 12 + 7, 2 ** 40, 987654321012, 2 ** 53 + 1, 3 * 10 ** 15]
    # (inter, est only, gt only): IoU = inter / (inter + est only + gt only)
    for k, (inter, eo, go) in enumerate([(20, 10, 10), (30, 10, 10), (70, 0, 30), (40, 5, 5), (90, 5, 5)]):
        s.add(inter, k + 1, big[k], True)
        s.add(eo, k + 1, 0, True)
        s.add(go, 0, big[k], True)
    s.add(10, 0, 77, 5)                      # ground-truth instance, moving fraction exactly 1/2 -> class 0, nothing estimated on it
    s.add(12, 9, 0, 6)                       # estimated instance with the same tie -> class 0
    s.add(40, 20, 5000000000, 0)             # a static pair, IoU 40 / 56
    s.add(16, 20, 0, 0)
    s.add(50, 21, 6000000000, 0)             # estimated moving (class 1) on a ground-truth static instance: never compared
    s.add(60, 21, 0, True)
    s.add(25, 0, 6000000000, 0)
    s.add(3000, 0, 0, 300)                   # background on both sides
    return s


def noisy_scene(rng, n_inst, n_bg):
    """Random instances with large sparse ids; the estimate splits, merges, drops and invents."""
    s = Scene()
    ids = rng.choice(np.arange(1, 2 ** 20), n_inst, replace=False).astype(np.int64) * 1000003 + 2 ** 33
    for k, gid in enumerate(ids):
        n = int(rng.randint(30, 900))
        moving = rng.rand() < 0.6
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.randint(0, 3)), replace=False)) if n > 3 else []
        parts = np.diff(np.concatenate([[0], cuts, [n]])).astype(int)
        for j, m in enumerate(parts):
            est = 0 if rng.rand() < 0.15 else (k // 2 + 1 if rng.rand() < 0.3 else 100 + 3 * k + j)     # dropped / merged with the neighbour / split
            s.add(int(m), est, int(gid), int(round(m * (0.93 if moving else 0.04))))
    for k in range(6):                                                                                 # invented clusters on background
        s.add(int(rng.randint(15, 200)), 900 + k, 0, bool(k % 2))
    s.add(n_bg, 0, 0, n_bg // 20)
    return s


def static_gt_scene():
    """Class 1 has estimated instances but no ground-truth instance."""
    s = Scene()
    s.add(80, 1, 11, 0)
    s.add(20, 0, 11, 0)
    s.add(70, 2, 12, 2)
    s.add(45, 3, 0, True)
    s.add(30, 4, 12, True)        # moving estimate on a static instance
    s.add(30, 4, 0, True)
    s.add(800, 0, 0, 0)
    return s


def no_est_scene():
    s = Scene()
    s.add(60, 0, 2 ** 45 + 3, True)
    s.add(40, 0, 8, 0)
    s.add(500, 0, 0, 40)
    return s


def no_gt_scene():
    s = Scene()
    s.add(55, 5, 0, True)
    s.add(35, 6, 0, 0)
    s.add(400, 0, 0, 10)
    return s


def nan_scene():
    """Only moving instances: class 0 is empty on both sides, so its entries print as nan."""
    s = Scene()
    s.add(30, 1, 100, True)
    s.add(10, 1, 0, True)
    s.add(10, 0, 100, True)
    s.add(25, 2, 200, True)
    s.add(100, 0, 0, 0)
    return s


def assemble(scenes, seed):
    rng = np.random.RandomState(seed)
    parts = [s.arrays(rng) for s in scenes]
    est, gt, mos = (np.concatenate([p[i] for p in parts]) for i in range(3))
    batch = np.concatenate([np.full(len(p[0]), b, np.int32) for b, p in enumerate(parts)])
    return est, gt, mos, batch


def facts(est, gt, mos):
    """Brute-force facts about one sample, in exact fractions: {id: (class, moving fraction)} per side, {(est id, gt id): IoU} for pairs of equal class."""
    def side(ids):
        out = {}
        for u in np.unique(ids):
            if u != 0:
                frac = Fraction(int(mos[ids == u].sum()), int((ids == u).sum()))
                out[int(u)] = (1 if frac > Fraction(1, 2) else 0, frac)
        return out
    e, g = side(est), side(gt)
    iou = {}
    for a, (ca, _) in e.items():
        for b, (cb, _) in g.items():
            if ca == cb:
                inter = int(((est == a) & (gt == b)).sum())
                iou[(a, b)] = Fraction(inter, int(((est == a) | (gt == b)).sum()))
    return e, g, iou


def check_edge_cases(est, gt, mos, batch):
    n_b = int(batch.max()) + 1
    assert n_b >= 3
    per = [facts(est[batch == b], gt[batch == b], mos[batch == b]) for b in range(n_b)]
    assert int(gt.max()) > 2 ** 53 and len(np.unique(gt)) < 100                                          # sparse large ids
    assert any(f == Fraction(1, 2) for e, g, _ in per for _, f in g.values())                            # a tie of the moving fraction, ground truth
    assert any(f == Fraction(1, 2) for e, g, _ in per for _, f in e.values())                            # ... and estimate
    best = [max([v for (a, _), v in iou.items() if a == ea], default=None) for e, g, iou in per for ea in e]
    for want in (Fraction(1, 2), Fraction(3, 5), Fraction(7, 10), Fraction(4, 5), Fraction(9, 10)):
        assert want in best, want                                                                        # as the BEST match of an estimated instance
    assert any(any(c == 1 for c, _ in e.values()) and not any(c == 1 for c, _ in g.values()) and g for e, g, _ in per)   # class 1: estimates, no ground truth
    assert any(not e and g for e, g, _ in per)                                                           # no estimated instance
    assert any(e and not g for e, g, _ in per)                                                           # all-zero ground truth
    for c in (0, 1):                                                                                     # no nan in the text
        assert any(cc == c for e, g, _ in per for cc, _ in g.values()) and any(cc == c for e, g, _ in per for cc, _ in e.values())


def run_reference(est, gt, mos, batch):
    ref_harness.install()
    if not hasattr(np, 'float'):
        np.float = float                                             # toolbox/cluster_eval.py:51-52
    from toolbox.cluster_eval import ClusterEvaluation
    with tempfile.TemporaryDirectory() as tmp:
        ev = ClusterEvaluation({'save_dir': tmp})
        e, g, m, t = torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mos).float(), torch.from_numpy(batch.astype(np.int64))
        for b in range(int(t.max() + 1)):                            # libs/loss.py:267-270
            sel = t == b
            ev(e[sel], g[sel], m[sel])
        with np.errstate(all='ignore'):
            ev.final_eval()
        ev.LOG_FOUT.close()
        text = open(os.path.join(tmp, 'cluster_eval.txt')).read()
    out = {'total_gt_inst': np.asarray(ev.total_gt_inst, np.float64), 'text': np.array(text)}
    for c in range(2):
        out['all_mean_cov_%d' % c] = np.asarray(ev.all_mean_cov[c], np.float64)
        out['all_mean_weighted_cov_%d' % c] = np.asarray(ev.all_mean_weighted_cov[c], np.float64)
        for thr in THRESHOLDS:
            out['tps_%s_%d' % (thr, c)] = np.asarray(ev.tpsins['@%s' % thr][c], np.float64)
            out['fps_%s_%d' % (thr, c)] = np.asarray(ev.fpsins['@%s' % thr][c], np.float64)
    return out


def gen_cluster_eval(save):
    rng = np.random.RandomState(11)
    est, gt, mos, batch = assemble([exact_scene(), noisy_scene(rng, 22, 9000), static_gt_scene(), no_est_scene(), no_gt_scene()], 12)
    check_edge_cases(est, gt, mos, batch)
    arrays = {'inst_est': est, 'inst_gt': gt, 'mos': mos, 'batch': batch}
    arrays.update(run_reference(est, gt, mos, batch))
    assert 'nan' not in str(arrays['text'])
    est2, gt2, mos2, batch2 = assemble([nan_scene()], 13)
    arrays.update({'nan_inst_est': est2, 'nan_inst_gt': gt2, 'nan_mos': mos2, 'nan_batch': batch2})
    arrays.update({'nan_' + k: v for k, v in run_reference(est2, gt2, mos2, batch2).items()})
    assert 'nan' in str(arrays['nan_text'])
    save('cluster_eval', **arrays)


if __name__ == '__main__':
    def save(name, **arrays):
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **arrays)
        print(name, {k: np.asarray(v).shape for k, v in arrays.items()}, os.path.getsize(os.path.join(HERE, name + '.npz')), 'bytes')
    gen_cluster_eval(save)
