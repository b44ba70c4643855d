"""Time the ICP pose refinement (include/pcacc.h C3, pcaccumulation_amd/icp.py) at its two call sites and, beside it on the same machine, what
the reference does on these inputs: the device -> host round trip of the points plus a KD-tree point-to-point ICP on 16 threads
(scipy.spatial.cKDTree standing in for Open3D's KD-tree, the same float64 Umeyama update and convergence rule: tests/icp_reference.py).
  ego       the benchmark's shape: 5 frames x 160 k points, about 80 % background, B = 1 and 4, threshold 0.1, 50 iterations at most
  instance  a few hundred instances of a few hundred points over 5 frames, threshold 0.15
GPU legs: device events around the launches of one call (warm-up first), median over --iters.  Results go to --out.  Nothing is gated on them.
Usage: python tools/bench_icp.py [--iters 5] [--instances 300] [--no-baseline] [--out profiles/icp_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def rigid(rng, deg, shift):
    import icp_reference
    return icp_reference.rigid(rng, deg, shift)


def ego_scene(seed, B, T=5, n_frame=160000, bg=0.8):
    """Frame 0 of a sample: points on a ground sheet and on walls inside +-50 m; frame t: 80 % of them moved by a small rigid motion with 1 cm of
    noise (the background the refinement aligns), the rest scattered (foreground, masked out).  Returns points, sample * T + frame, background, poses."""
    rng = np.random.RandomState(seed)
    pts, frame, back, init = [], [], [], []
    for b in range(B):
        base = np.concatenate((rng.uniform(-50, 50, (n_frame, 2)), rng.uniform(-2, 2, (n_frame, 1)) ** 3 / 4), axis=1)
        for t in range(T):
            M = rigid(rng, 0.5 * t, 0.1 * t)
            p = base @ np.linalg.inv(M)[:3, :3].T + np.linalg.inv(M)[:3, 3] + (rng.randn(n_frame, 3) * 0.01 if t else 0)
            is_bg = rng.rand(n_frame) < bg
            p[~is_bg] += rng.uniform(-3, 3, ((~is_bg).sum(), 3))
            pts.append(p); frame.append(np.full(n_frame, b * T + t)); back.append(is_bg)
            init.append(rigid(rng, 0.05, 0.03) @ M if t else np.eye(4))       # the network's estimate: the motion, a few centimetres off
    return (np.concatenate(pts).astype(np.float32), np.concatenate(frame), np.concatenate(back), np.stack(init).astype(np.float32))


def instance_scene(seed, K, T=5):
    rng = np.random.RandomState(seed)
    pts, lab, frm = [], [], []
    for k in range(K):
        n = rng.randint(100, 600)
        base = rng.uniform(-1.5, 1.5, (n, 3)) * [1, 0.6, 0.5] + rng.uniform(-40, 40, 3) * [1, 1, 0]
        for t in range(T):
            M = rigid(rng, 0.3, 0.04) if t else np.eye(4)
            keep = rng.rand(n) < 0.8
            c = base[keep].mean(0)
            p = (base[keep] - c) @ M[:3, :3].T + M[:3, 3] + c
            pts.append(p); lab.append(np.full(p.shape[0], k)); frm.append(np.full(p.shape[0], t))
    order = rng.permutation(sum(p.shape[0] for p in pts))
    return np.concatenate(pts).astype(np.float32)[order], np.concatenate(lab)[order], np.concatenate(frm)[order]


def kdtree_icp(src, tgt_tree, tgt, threshold, init, max_iter, workers=16):
    """tests/icp_reference.icp with the brute-force search replaced by a KD-tree query on `workers` threads."""
    import icp_reference as ref

    def evaluate(s):
        d, j = tgt_tree.query(s, k=1, distance_upper_bound=threshold, workers=workers)
        ok = np.isfinite(d)
        k = int(ok.sum())
        return np.where(ok, j, -1), (k / s.shape[0] if s.shape[0] else 0.0), (float(np.sqrt((d[ok] ** 2).sum() / k)) if k else 0.0)
    s = ref.transform(init, src.astype(np.float64))
    T = np.eye(4)
    idx, fit, rmse = evaluate(s)
    for _ in range(max_iter):
        sel = idx >= 0
        up = ref.umeyama(s[sel], tgt[idx[sel]])
        T, s = up @ T, ref.transform(up, s)
        prev = (fit, rmse)
        idx, fit, rmse = evaluate(s)
        if abs(prev[0] - fit) < 1e-6 and abs(prev[1] - rmse) < 1e-6:
            break
    return T @ init


def gpu_time(fn, iters):
    import torch
    fn()                                                                      # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--instances', type=int, default=300)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icp_bench.txt'))
    a = ap.parse_args()
    import torch
    from scipy.spatial import cKDTree
    from pcaccumulation_amd import icp
    from pcaccumulation_amd.tpointnet import reconstruct_sequence
    dev = torch.device('cuda:0')
    lines = ['tools/bench_icp.py --iters %d --instances %d   (%s; GPU: device events around one call, median; host: perf_counter)'
             % (a.iters, a.instances, torch.cuda.get_device_name(0))]
    T = 5
    for B in (1, 4):
        pts, frame, back, init = ego_scene(B, B)
        t_pts, t_frame, t_back, t_init = (torch.from_numpy(x).to(dev) for x in (pts, frame, back, init))
        med, times = gpu_time(lambda: icp.refine_ego_poses(t_pts, t_frame, t_back, t_init, B, T, 0.1, 50), a.iters)
        refined, status = icp.refine_ego_poses(t_pts, t_frame, t_back, t_init, B, T, 0.1, 50)
        line = 'ego B=%d (%d points): GPU %.2f ms per call (%s)' % (B, pts.shape[0], med, ' '.join('%.2f' % t for t in times))
        if not a.no_baseline:
            t0 = time.perf_counter()
            h_pts, h_init = t_pts.cpu().numpy(), t_init.cpu().numpy().astype(np.float64)      # the reference's round trip
            worst = 0.0
            for b in range(B):
                tgt = h_pts[(frame == b * T) & back].astype(np.float64)
                tree = cKDTree(tgt)
                for t in range(1, T):
                    want = kdtree_icp(h_pts[(frame == b * T + t) & back], tree, tgt, 0.1, h_init[b * T + t], 50)
                    worst = max(worst, float(np.abs(refined[b * T + t].cpu().numpy() - want).max()))
            host = (time.perf_counter() - t0) * 1e3
            line += ' | host round trip + 16-thread cKDTree ICP %.0f ms | largest pose difference %.2e' % (host, worst)
        lines.append(line)
        print(line, flush=True)
    pts, lab, frm = instance_scene(9, a.instances)
    t_pts, t_lab, t_frm = (torch.from_numpy(x).to(dev) for x in (pts, lab, frm))
    pose0 = torch.eye(4, device=dev).repeat(a.instances, T, 1, 1)
    med, times = gpu_time(lambda: icp.refine_instance_poses(t_pts, t_frm, t_lab, pose0, 0.15, 50), a.iters)
    got = icp.refine_instance_poses(t_pts, t_frm, t_lab, pose0, 0.15, 50)[0].cpu().numpy()
    line = 'instance K=%d (%d points, %d jobs): GPU %.2f ms per call (%s)' % (a.instances, pts.shape[0], a.instances * (T - 1), med, ' '.join('%.2f' % t for t in times))
    if not a.no_baseline:
        t0 = time.perf_counter()
        rec = reconstruct_sequence(t_pts, t_frm, t_lab, pose0, T).cpu().numpy()
        worst = 0.0
        for k in range(a.instances):                                          # models/alignnet.py:107-111: one mask and one round trip per instance
            sel = lab == k
            p, f = rec[sel].astype(np.float64), frm[sel]
            tgt = p[f == 0]
            tree = cKDTree(tgt)
            for t in range(1, T):
                want = kdtree_icp(p[f == t], tree, tgt, 0.15, np.eye(4), 50)
                worst = max(worst, float(np.abs(got[k, t] - want).max()))
        host = (time.perf_counter() - t0) * 1e3
        line += ' | host round trip + 16-thread cKDTree ICP %.0f ms | largest pose difference %.2e' % (host, worst)
    lines.append(line)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
