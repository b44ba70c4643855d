#!/usr/bin/env python
"""Emit the golden vectors under tests/golden/ by running the REFERENCE itself (imported read-only
from /root/reference, CPU, this container only -- see ref_harness.py for the stand-ins of absent
third-party modules).  The fixtures are data: seeds / inputs and the reference's outputs.

    python tests/golden/make_golden.py [ops] [model] [chamfer] [aniso]

Inputs that are large are regenerated from a seed by pcaccumulation_amd.synthetic (numpy legacy
RandomState, byte-stable); only small tensors, samples and digests are stored.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.install()
from pcaccumulation_amd.config import default_config  # noqa: E402
from pcaccumulation_amd.synthetic import make_sequence, attach_voxels, fill_state_dict_  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save(name, **kw):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **kw)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


def vox_points(seed, n, cfg, frac_out=0.1):
    """Random points for the voxeliser incl. out-of-range and on-edge values."""
    rng = np.random.RandomState(seed)
    r = np.asarray(cfg['voxel_generator']['range'], np.float64)
    T = cfg['voxel_generator']['n_sweeps']
    lo, hi = r[:3], r[3:]
    span = hi - lo
    p = lo + rng.uniform(-frac_out / 2, 1 + frac_out / 2, (n, 3)) * span
    t = rng.randint(0, T, n)
    edge = rng.randint(0, n, 32)                      # exact cell edges and range limits
    p[edge[:8], 0] = lo[0]
    p[edge[8:16], 0] = hi[0]
    p[edge[16:24], 1] = lo[1] + 0.25 * rng.randint(0, int(span[1] / 0.25), 8)
    p[edge[24:], 2] = hi[2]
    return np.concatenate([p, t[:, None]], axis=1).astype(np.float32)


def gen_ops():
    from libs.voxel_generator import Voxelization, points_to_voxel
    from models.pillar_encoder import (PillarFeatureNet, scatter_point_pillar, inverse_scatter_point_pillar,
                                       ungrid, temporal_ungrid)
    from models.motionnet import MotionNet
    from models.egomotion import EgoMotionHead
    from toolbox.utils import square_distance
    from toolbox.register_utils import kabsch_transformation_estimation, rotation_error, translation_error
    from torch_scatter import scatter
    from libs.loss import compute_iou
    from toolbox.sf_eval_utils import compute_sf_metrics_torch

    # ---- A1 voxelisation ------------------------------------------------------------------
    cfg_s = default_config('waymo', 'val', n_sweeps=3, xy_range=8)
    pts = vox_points(1, 3000, cfg_s)
    v = Voxelization(cfg_s['voxel_generator'])(pts)
    vg = cfg_s['voxel_generator']
    capped = points_to_voxel(pts, np.array(vg['voxel_size'], np.float32), np.array(vg['range'], np.float32),
                             vg['n_sweeps'], max_voxels=200)
    save('vox_small', points=pts, coordinates=v['coordinates'], num_voxels=v['num_voxels'], shape=v['shape'],
         point_to_voxel_map=v['point_to_voxel_map'], cap_coordinates=capped[0], cap_p2v=capped[2],
         cap_num_points=capped[1])

    cfg_w = default_config('waymo', 'val')
    pts_w = vox_points(2, 100000, cfg_w, frac_out=0.02)
    vw = Voxelization(cfg_w['voxel_generator'])(pts_w)
    save('vox_waymo', seed=2, n=100000, points_sha=sha(pts_w), num_voxels=vw['num_voxels'], shape=vw['shape'],
         coordinates_sha=sha(vw['coordinates']), p2v_sha=sha(vw['point_to_voxel_map']),
         coordinates_head=vw['coordinates'][:64], p2v_head=vw['point_to_voxel_map'][:256, 0],
         p2v_tail=vw['point_to_voxel_map'][-256:, 0])

    # ---- A3/A4 pooling + PFN on a collated batch of two small samples -------------------------
    vox = rh.voxeliser(cfg_s)
    samples = [attach_voxels(make_sequence(s, 3, 1500, cfg_s), vox) for s in (10, 11)]
    inp = rh.collate(samples)
    points = inp['input_points'].float()
    p2v = inp['point_to_voxel_map'].long()[:, 0]
    pillar_mean = scatter(points, p2v, dim=0, reduce='mean')
    fb_sub = scatter(inp['fb_labels'], p2v, dim=0, reduce='max')
    pfn = PillarFeatureNet(cfg_s['pillar_encoder']).eval()
    fill_state_dict_(pfn)
    with torch.no_grad():
        pfn_out = pfn(points, p2v, inp['coordinates'], pillar_mean, inp['time_indice'])
    save('segops', seeds=np.array([10, 11]), pillar_mean=pillar_mean.numpy(), fb_labels_sub=fb_sub.numpy(),
         pfn_out=pfn_out.numpy(), coordinates=inp['coordinates'].numpy(),
         p2v=inp['point_to_voxel_map'].numpy())

    # ---- A5/A6 scatter / inverse scatter ----------------------------------------------------------
    B = 2
    shape = inp['shape'][0]
    rng = np.random.RandomState(3)
    feats = torch.from_numpy(rng.randn(inp['coordinates'].shape[0], 4).astype(np.float32))
    canvas = scatter_point_pillar(feats, inp['coordinates'], B, shape)
    icanvas = torch.from_numpy(rng.randint(0, 5, (B, 1, int(shape[3]), int(shape[1]), int(shape[0]))))
    inv = inverse_scatter_point_pillar(icanvas, inp['coordinates'], B, shape)
    save('scatter', feats=feats.numpy(), canvas=canvas.numpy(), icanvas=icanvas.numpy(), inverse=inv.numpy())

    # ---- A11 ungrid / temporal_ungrid ----------------------------------------------------------
    fmap = torch.from_numpy(rng.randn(2, 4, 16, 16).astype(np.float32))
    K = 700                                              # > H*W so the reference builds extra fake grids
    upts = torch.from_numpy(rng.uniform(-9.5, 9.5, (K, 3)).astype(np.float32))
    uti = torch.from_numpy(np.stack([np.sort(rng.randint(0, 2, K)), rng.randint(0, 3, K)], 1).astype(np.float64))
    ug = ungrid(fmap, upts.clone(), [-8, -8, -2, 8, 8, 6], uti)
    fmap_t = torch.from_numpy(rng.randn(2, 3, 4, 16, 16).astype(np.float32))
    tug = temporal_ungrid(fmap_t, upts.clone(), [-8, -8, -2, 8, 8, 6], uti)
    upts512 = upts[:512][uti[:512, 0] == 0][:256]        # K % (H*W) == 0 corner case (one batch, 256 points)
    ug256 = ungrid(fmap[:1], upts512.clone(), [-8, -8, -2, 8, 8, 6], uti[:upts512.shape[0]] * 0)
    save('ungrid', fmap=fmap.numpy(), points=upts.numpy(), time_indice=uti.numpy(), out=ug.numpy(),
         fmap_t=fmap_t.numpy(), out_t=tug.numpy(), points256=upts512.numpy(), out256=ug256.numpy())

    # ---- A9 warp_feats / transform_points ------------------------------------------------------
    net = MotionNet(cfg_s)
    bev = torch.from_numpy(rng.randn(2, 3, 4, 64, 64).astype(np.float32))
    poses = torch.eye(4).repeat(2, 3, 1, 1)
    for b in range(2):
        for t in range(1, 3):
            a = rng.uniform(-0.2, 0.2)
            poses[b, t, :2, :2] = torch.tensor([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            poses[b, t, :3, 3] = torch.from_numpy(rng.uniform(-2, 2, 3).astype(np.float32))
    warped = net.warp_feats(bev, poses)
    tp = net.transform_points(points.clone(), inp['time_indice'], poses)
    save('warp', bev=bev.numpy(), poses=poses.numpy(), warped=warped.numpy(), transformed=tp.numpy(),
         seeds=np.array([10, 11]))

    # ---- A8 ego-motion pieces ----------------------------------------------------------------
    cfg_e = default_config('waymo', 'val', n_sweeps=3, xy_range=8)
    cfg_e['pose_estimation']['n_kpts'] = 64
    head = EgoMotionHead(cfg_e)
    with torch.no_grad():
        head.alpha.fill_(-1.3)
        head.beta.fill_(-2.1)
    a = torch.from_numpy(rng.randn(1, 50, 3).astype(np.float32))
    bb = torch.from_numpy(rng.randn(1, 70, 3).astype(np.float32))
    sq = square_distance(a, bb)
    aff = torch.from_numpy((rng.randn(1, 64, 64) * 3).astype(np.float32))
    sk = head.sinkhorn(aff, n_iters=3)
    x1 = torch.from_numpy(rng.randn(1, 64, 3).astype(np.float32))
    ang = 0.4
    Rt = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=torch.float32)
    x2 = x1 @ Rt.T + torch.tensor([0.3, -0.2, 0.1]) + 0.01 * torch.from_numpy(rng.randn(1, 64, 3).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0, 1, (1, 64)).astype(np.float32))
    kr, kt, _, _ = kabsch_transformation_estimation(x1, x2, weights=w)
    # pairwise with n_source > n_kpts (randperm path) and n_target < n_kpts (clamped arange path)
    fs = torch.nn.functional.normalize(torch.from_numpy(rng.randn(150, 16).astype(np.float32)), dim=1)
    ft = torch.nn.functional.normalize(torch.from_numpy(rng.randn(40, 16).astype(np.float32)), dim=1)
    cs = torch.from_numpy(rng.uniform(-3, 3, (150, 3)).astype(np.float32))
    ct = torch.from_numpy(rng.uniform(-3, 3, (40, 3)).astype(np.float32))
    choices = []
    orig = torch.randperm

    def rec(n, *a_, **k_):
        p = orig(n, *a_, **k_)
        choices.append(p.numpy().copy())
        return p
    torch.randperm = rec
    torch.manual_seed(7)
    with torch.no_grad():
        pose, perm = head.pairwise_ego_motion_estimation(fs, ft, cs, ct, 0.1)
    torch.randperm = orig
    choice_s = choices[0][:64]
    choice_t = np.arange(64)
    choice_t[40:] = 39
    r1 = torch.from_numpy(np.stack([np.linalg.qr(rng.randn(3, 3))[0] for _ in range(5)]).astype(np.float32))
    r1 = r1 * torch.sign(torch.det(r1))[:, None, None]
    r2 = torch.roll(r1, 1, 0)
    t1 = torch.from_numpy(rng.randn(5, 3, 1).astype(np.float32))
    t2 = torch.from_numpy(rng.randn(5, 3, 1).astype(np.float32))
    save('ego', sq_a=a.numpy(), sq_b=bb.numpy(), sq=sq.numpy(), aff=aff.numpy(), sinkhorn=sk.numpy(),
         x1=x1.numpy(), x2=x2.numpy(), w=w.numpy(), kabsch_r=kr.numpy(), kabsch_t=kt.numpy(),
         fs=fs.numpy(), ft=ft.numpy(), cs=cs.numpy(), ct=ct.numpy(), choice_s=choice_s, choice_t=choice_t,
         pose=pose.numpy(), perm=perm.numpy(), alpha=-1.3, beta=-2.1, duration=0.1, max_speed=30, seed=7,
         r1=r1.numpy(), r2=r2.numpy(), rot_err=rotation_error(r1, r2).numpy(), t1=t1.numpy(), t2=t2.numpy(),
         trans_err=translation_error(t1, t2).numpy())

    # ---- M1 / M3 metric definitions -------------------------------------------------------------
    pred = torch.from_numpy(rng.randint(0, 2, 5000))
    gt = torch.from_numpy(rng.randint(0, 2, 5000))
    iou = compute_iou(pred, gt, 2, -1)
    epe = torch.from_numpy(np.abs(rng.randn(4000)).astype(np.float32) * 0.2)
    rel = torch.from_numpy(np.abs(rng.randn(4000)).astype(np.float32) * 0.2)
    sf = compute_sf_metrics_torch(epe, rel)
    save('metrics', pred=pred.numpy(), gt=gt.numpy(), intersection=iou['intersection'], union=iou['union'],
         pred_positives=iou['pred_positives'], gt_positives=iou['gt_positives'], epe=epe.numpy(), rel=rel.numpy(),
         sf=np.array([sf['EPE3D'][0], sf['EPE3D_med'], sf['Acc3DS'][0], sf['Acc3DR'][0], sf['Outlier'][0],
                      sf['ROutlier'][0]]))


if __name__ == '__main__':
    what = sys.argv[1:] or ['ops', 'chamfer', 'model']
    if 'ops' in what:
        gen_ops()
    if 'chamfer' in what:
        from make_golden_chamfer import gen_chamfer
        gen_chamfer(save)
    if 'model' in what:
        from make_golden_model import gen_model
        gen_model(save, sha)
    if 'aniso' in what:
        from make_golden_aniso import gen_aniso
        gen_aniso(save)
