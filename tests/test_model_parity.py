"""Whole-path parity: the product MotionNet (+ FuseLoss) against the golden vectors the reference produced
on the same seeded inputs and closed-form weights.

Two legs share one body:
  * `-m "not gpu"`: host logic only -- pcaccumulation_amd.native is replaced by the oracle-backed test double
    (oracle/cpu_backend.py) so that module wiring, layouts, autograd wrappers and result keys are checked here;
  * `-m gpu`: the real HIP library on cuda:0, fp32 compute, then bf16 compute with tolerances on metrics only.
Tolerance from BASELINE.json's north_star: metrics (mos_iou, ego rot/trans error, scene-flow EPE) within 1e-3;
integer outputs bit-exact."""
import numpy as np
import pytest
import torch

from helpers import make_batch
from pcaccumulation_amd.config import default_config
from pcaccumulation_amd.loss import FuseLoss, scene_flow_epe
from pcaccumulation_amd.motionnet import MotionNet
from pcaccumulation_amd.synthetic import fill_state_dict_


def _to(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _build(g, cfg, dev, train):
    inp = make_batch(cfg, [int(s) for s in g['seeds']], int(g['n_frames']), int(g['pts_per_frame']))
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in zip(g['tweak_keys'], g['tweak_vals']):
            sd[str(k)] += torch.from_numpy(v)
    model = model.to(dev).train(train)
    if dev.type == 'cuda':
        model.channels_last_()
    return model, _to(inp, dev)


def _first_sample(inp):
    sel = inp['time_indice'][:, 0] == 0
    out = {k: inp[k][sel] for k in ('input_points', 'time_indice', 'inst_labels')}
    out['ego_motion_gt'] = inp['ego_motion_gt']
    out['inst_motion_gt'] = inp['inst_motion_gt']
    return out, sel


def _check_metrics(g, out, stats, inp, n_frames, tol):
    assert abs(out['ego_rot_error'] - float(g['ego_rot_error'])) < tol['ego']
    assert abs(out['ego_trans_error'] - float(g['ego_trans_error'])) < tol['ego']
    i, u = stats['mos_metric']['intersection'], stats['mos_metric']['union']
    assert abs(float((i / (u + 1e-20)).mean()) - float(g['mos_iou'])) < tol['iou']
    s0, sel = _first_sample(inp)
    s0['input_points'] = s0['input_points'].float()
    epe = scene_flow_epe({'rec_est': out['rec_est'][sel]}, s0, n_frames)
    assert abs(float(epe.mean()) - float(g['epe_mean'])) < tol['epe']
    return epe


def _tiny_val(dev, golden, compute_dtype='fp32'):
    g = golden('model_tiny_val')
    cfg = default_config('waymo', 'val', n_sweeps=3, xy_range=8)
    cfg['misc']['compute_dtype'] = compute_dtype
    model, inp = _build(g, cfg, dev, train=False)
    loss_fn = FuseLoss(cfg['loss'])
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
        stats = loss_fn(out, inp)
    return g, out, stats, inp


def _tiny_val_aniso(dev, golden):
    """_tiny_val on the non-square grid with non-square cells (helpers.aniso_cfg; tests/golden/make_golden_aniso.py)."""
    from helpers import aniso_batch
    g = golden('model_tiny_val_aniso')
    cfg, inp = aniso_batch([int(s) for s in g['seeds']], int(g['n_frames']), int(g['pts_per_frame']))
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in zip(g['tweak_keys'], g['tweak_vals']):
            sd[str(k)] += torch.from_numpy(v)
    model = model.to(dev).eval()
    if dev.type == 'cuda':
        model.channels_last_()
    inp = _to(inp, dev)
    loss_fn = FuseLoss(cfg['loss'])
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
        stats = loss_fn(out, inp)
    return g, out, stats, inp


def _no_flips(g, out):
    """The fixture's smallest |fg - bg| logit gap at an occupied pillar (fb_margin) is at least 4 x the tolerance on fb_seg_est: a result within
    tolerance cannot flip a point, so the comparisons behind `if flips == 0` in _assert_tiny_val_fp32 always run."""
    assert float(g['fb_margin']) >= 2e-3
    assert int((out['fb_est_per_points'].cpu().numpy() != g['fb_est_per_points']).sum()) == 0


def _assert_tiny_val_fp32(g, out, stats, inp, atol):
    c = lambda t: t.detach().float().cpu().numpy()
    assert np.array_equal(c(out['fb_seg_gt']), g['fb_seg_gt'])
    assert np.array_equal(c(out['occ_map']), g['occ_map'])
    np.testing.assert_allclose(c(out['fb_seg_est']), g['fb_seg_est'], rtol=1e-3, atol=atol)
    # argmax-derived integer outputs: identical except where the two logits are within the conv tolerance
    flips = (out['fb_est_per_points'].cpu().numpy() != g['fb_est_per_points']).mean()
    assert flips <= 1e-3
    np.testing.assert_allclose(c(out['ego_motion_est']), g['ego_motion_est'], atol=10 * atol)
    np.testing.assert_allclose(c(out['ego_motion_gt']), g['ego_motion_gt'], atol=1e-5)
    np.testing.assert_allclose(c(out['transformed_points']), g['transformed_points'], atol=100 * atol)
    np.testing.assert_allclose(np.stack([c(p.sum(2)[0]) for p in out['perm_matrix']]), g['perm_rowsum'], atol=10 * atol)
    if flips == 0:
        np.testing.assert_allclose(c(out['mos_est']), g['mos_est'], rtol=1e-2, atol=100 * atol)
        np.testing.assert_allclose(c(out['offset_est']), g['offset_est'], rtol=1e-2, atol=100 * atol)
        np.testing.assert_allclose(c(out['rec_est']), g['rec_est'], rtol=1e-2, atol=100 * atol)
        np.testing.assert_allclose(c(out['inst_pose_est']), g['inst_pose_est'], rtol=1e-2, atol=100 * atol)
        assert np.array_equal(out['inst_labels_adjusted'].cpu().numpy(), g['inst_labels_adjusted'])
        for k in ('loss', 'fb_loss', 'mos_loss', 'offset_loss', 'obj_loss', 'perm_loss', 'ego_l1_loss', 'inst_l2_error'):
            got = float(stats[k]) if k in stats else float(out[k])
            assert abs(got - float(g[k])) < 1e-3 * max(1.0, abs(float(g[k]))), k
        assert np.allclose(stats['fb_metric']['intersection'], g['fb_metric_intersection'], atol=2e-3)
    expected_keys = {'fb_seg_gt', 'occ_map', 'fb_seg_est', 'fb_est_per_points', 'ego_l1_loss', 'ego_l2_loss', 'ego_rot_error',
                     'ego_trans_error', 'perm_matrix', 'ego_motion_est', 'ego_motion_gt', 'transformed_points', 'mos_est',
                     'offset_est', 'rec_est', 'tpointnet_loss_terms', 'inst_l2_error', 'dynamic_inst_l2_error',
                     'inst_labels_adjusted', 'inst_pose_est', 'sub_rec_est'}
    assert expected_keys <= set(out.keys())


def _tiny_train(dev, golden):
    g = golden('model_tiny_train')
    cfg = default_config('waymo', 'train', n_sweeps=3, xy_range=8)
    model, inp = _build(g, cfg, dev, train=True)
    loss_fn = FuseLoss(cfg['loss'])
    torch.manual_seed(int(g['fwd_seed']))
    out = model(inp)
    stats = loss_fn(out, inp)
    stats['loss'].backward()
    return g, model, out, stats, inp


def _assert_tiny_train(g, model, out, stats, rtol):
    assert abs(float(stats['loss']) - float(g['loss'])) < rtol * abs(float(g['loss']))
    grads = dict(model.named_parameters())
    names = [str(n) for n in g['grad_names']]
    assert names == list(grads.keys())
    bad = []
    # Layers upstream of STPN's max-over-T / max-pools: the warped features carry fp32 rounding noise, the empty BEV
    # regions are near-ties across frames, so WHICH frame/pixel receives the gradient differs between any two
    # implementations although the loss agrees to 1e-7.  Their gradient norms are compared at 2 %.
    loose = ('motionhead.init_conv', 'motionhead.down_convs', 'motionhead.up_convs')
    for n, ref in zip(names, g['grad_norms']):
        p = grads[n]
        got = float(p.grad.norm()) if p.grad is not None else 0.0
        tol = 2e-2 if n.startswith(loose) else 5 * rtol
        if abs(got - ref) > tol * max(abs(ref), 1e-3):
            bad.append((n, got, float(ref)))
    assert not bad, bad[:8]
    np.testing.assert_allclose(model.semseg_head.seg_head[1].running_mean.detach().cpu().numpy(), g['bn_running_mean'],
                               rtol=10 * rtol, atol=1e-4)


# ------------------------------------------------------------------------------------------------ CPU leg
@pytest.fixture
def double(monkeypatch):
    from oracle import cpu_backend
    cpu_backend.install(monkeypatch)
    return torch.device('cpu')


def test_state_dict_contract(golden):
    g = golden('state_dict_keys')
    sd = MotionNet(default_config('waymo', 'val')).state_dict()
    assert [str(k) for k in g['keys']] == list(sd.keys())
    assert [str(s) for s in g['shapes']] == [str(tuple(v.shape)) for v in sd.values()]
    assert [str(s) for s in g['dtypes']] == [str(v.dtype) for v in sd.values()]


def test_host_logic_tiny_val(double, golden):
    g, out, stats, inp = _tiny_val(double, golden)
    _assert_tiny_val_fp32(g, out, stats, inp, atol=1e-4)
    epe = _check_metrics(g, out, stats, inp, 3, dict(ego=1e-3, iou=1e-3, epe=1e-3))
    np.testing.assert_allclose(epe.numpy(), g['epe'], rtol=1e-3, atol=1e-3)


def test_host_logic_tiny_val_aniso(double, golden):
    g, out, stats, inp = _tiny_val_aniso(double, golden)
    assert tuple(out['fb_seg_est'].shape) == (2, 3, 2, 96, 64)
    _no_flips(g, out)
    _assert_tiny_val_fp32(g, out, stats, inp, atol=1e-4)
    _check_metrics(g, out, stats, inp, 3, dict(ego=1e-3, iou=1e-3, epe=1e-3))


def test_host_logic_tiny_train_backward(double, golden):
    g, model, out, stats, inp = _tiny_train(double, golden)
    _assert_tiny_train(g, model, out, stats, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ GPU leg
@pytest.mark.gpu
def test_gpu_tiny_val_fp32(golden):
    g, out, stats, inp = _tiny_val(torch.device('cuda:0'), golden)
    _assert_tiny_val_fp32(g, out, stats, inp, atol=5e-4)
    _check_metrics(g, out, stats, inp, 3, dict(ego=1e-3, iou=1e-3, epe=1e-3))


@pytest.mark.gpu
def test_gpu_tiny_val_aniso_fp32(golden):
    g, out, stats, inp = _tiny_val_aniso(torch.device('cuda:0'), golden)
    _no_flips(g, out)
    _assert_tiny_val_fp32(g, out, stats, inp, atol=5e-4)
    _check_metrics(g, out, stats, inp, 3, dict(ego=1e-3, iou=1e-3, epe=1e-3))


@pytest.mark.gpu
def test_gpu_tiny_train_backward_fp32(golden):
    g, model, out, stats, inp = _tiny_train(torch.device('cuda:0'), golden)
    _assert_tiny_train(g, model, out, stats, rtol=5e-3)


@pytest.mark.gpu
def test_gpu_waymo_val_fp32(golden):
    """BASELINE config c1 shape (5 x 20k points, 288 x 288 grid): metrics within 1e-3, integer structure bit-exact."""
    g = golden('model_waymo_val')
    cfg = default_config('waymo', 'val')
    dev = torch.device('cuda:0')
    model, inp = _build(g, cfg, dev, train=False)
    assert int(inp['num_voxels'][0]) == int(g['num_voxels'][0])
    loss_fn = FuseLoss(cfg['loss'])
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
        stats = loss_fn(out, inp)
    _check_metrics(g, out, stats, inp, 5, dict(ego=1e-3, iou=1e-3, epe=1e-3))
    idx = torch.from_numpy(g['sample_idx']).to(dev)
    np.testing.assert_allclose(out['transformed_points'][idx].cpu().numpy(), g['transformed_points'], atol=2e-3)
    assert (out['fb_est_per_points'][idx].cpu().numpy() != g['fb_est_per_points']).mean() < 2e-3
    assert abs(int(out['fb_est_per_points'].sum()) - int(g['fb_est_sum'])) <= 0.002 * int(g['fb_est_sum'])
    np.testing.assert_allclose(out['fb_seg_est'][0, :, :, ::8, ::8].cpu().numpy(), g['fb_seg_est_sample'], rtol=1e-3, atol=1e-3)


@pytest.mark.gpu
def test_gpu_tiny_val_bf16_metrics(golden):
    """bf16 canvas + bf16 conv stacks: tolerance on the metrics only (argmax masks may flip under bf16)."""
    g, out, stats, inp = _tiny_val(torch.device('cuda:0'), golden, compute_dtype='bf16')
    assert abs(out['ego_rot_error'] - float(g['ego_rot_error'])) < 0.5          # degrees; random-weight features
    i, u = stats['mos_metric']['intersection'], stats['mos_metric']['union']
    assert abs(float((i / (u + 1e-20)).mean()) - float(g['mos_iou'])) < 0.05
    assert (out['fb_est_per_points'].cpu().numpy() != g['fb_est_per_points']).mean() < 0.05


@pytest.mark.gpu
def test_gpu_vs_oracle_backend_ragged_batch(monkeypatch):
    """Ragged batch (samples with different point and pillar counts, T = 5, train mode incl. backward): the HIP library and
    the oracle-backed CPU backend under the SAME host code must agree -- every kernel is exercised in context at shapes the
    golden vectors do not cover."""
    from helpers import oracle_voxeliser
    from pcaccumulation_amd.dataloader import collate_fn
    from pcaccumulation_amd.synthetic import make_sequence, attach_voxels
    cfg = default_config('waymo', 'train', n_sweeps=5, xy_range=8)
    vox = oracle_voxeliser(cfg)
    samples = [attach_voxels(make_sequence(40, 5, 1400, cfg), vox), attach_voxels(make_sequence(41, 5, 700, cfg, mode='lidar'), vox),
               attach_voxels(make_sequence(42, 5, 2100, cfg), vox)]
    inp = collate_fn(samples)
    assert len(set(int(v) for v in inp['num_voxels'])) == 3

    def run(dev):
        torch.manual_seed(5)
        model = MotionNet(cfg)
        fill_state_dict_(model)
        with torch.no_grad():                                   # both classes of the fb head occur (see make_golden_model.py)
            model.semseg_head.seg_head[3].bias += torch.tensor([17.0, 0.0])
        model = model.to(dev).train()
        if dev.type == 'cuda':
            model.channels_last_()
        batch = _to(inp, dev)
        torch.manual_seed(6)
        out = model(batch)
        stats = FuseLoss(cfg['loss'])(out, batch)
        stats['loss'].backward()
        grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
        keep = {k: out[k].detach().cpu() for k in ('fb_seg_est', 'fb_est_per_points', 'transformed_points', 'mos_est', 'ego_motion_est')}
        return keep, float(stats['loss']), grads, out['ego_rot_error']

    gpu = run(torch.device('cuda:0'))
    from oracle import cpu_backend
    cpu_backend.install(monkeypatch)
    cpu = run(torch.device('cpu'))
    np.testing.assert_allclose(gpu[0]['fb_seg_est'].numpy(), cpu[0]['fb_seg_est'].numpy(), rtol=1e-3, atol=1e-3)
    assert (gpu[0]['fb_est_per_points'] != cpu[0]['fb_est_per_points']).float().mean() < 2e-3
    np.testing.assert_allclose(gpu[0]['ego_motion_est'].numpy(), cpu[0]['ego_motion_est'].numpy(), atol=5e-3)
    np.testing.assert_allclose(gpu[0]['transformed_points'].numpy(), cpu[0]['transformed_points'].numpy(), atol=5e-2)
    assert abs(gpu[1] - cpu[1]) < 5e-3 * abs(cpu[1])
    assert abs(gpu[3] - cpu[3]) < 1e-2
    for k in ('pillar_encoder.fc_pos.weight', 'pillar_encoder.blocks.2.fc_0.weight', 'unet.conv_final.weight',
              'motionhead.mos_seg.seg_head.3.weight', 'ego_feats_head.seg_head.3.weight'):
        g, c = gpu[2][k], cpu[2][k]
        assert abs(float(g.norm()) - float(c.norm())) < 3e-2 * max(float(c.norm()), 1e-3), k


def _no_foreground(dev):
    """MIN_POINTS gates (models/motionnet.py:11,222,243): with no foreground point at all the STPN and the TubeNet are skipped,
    mos_est defaults to class 0 / zero offsets, and FuseLoss still returns a finite loss that back-propagates."""
    from helpers import oracle_voxeliser
    from pcaccumulation_amd.dataloader import collate_fn
    from pcaccumulation_amd.synthetic import make_sequence, attach_voxels
    cfg = default_config('waymo', 'train', n_sweeps=3, xy_range=8)
    sample = attach_voxels(make_sequence(50, 3, 1200, cfg, n_inst=0), oracle_voxeliser(cfg))
    assert int(sample['fb_labels'].sum()) == 0
    inp = _to(collate_fn([sample]), dev)
    torch.manual_seed(0)
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        model.semseg_head.seg_head[3].bias += torch.tensor([1e4, 0.0])            # every pillar predicted background
    model = model.to(dev).train()
    out = model(inp)
    assert int(out['fb_est_per_points'].sum()) == 0
    assert 'tpointnet_loss_terms' not in out and 'inst_pose_est' not in out
    assert torch.equal(out['mos_est'].cpu(), torch.tensor([[1.0, 0.0]]).repeat(inp['input_points'].shape[0], 1))
    assert float(out['offset_est'].abs().sum()) == 0.0
    assert torch.equal(out['rec_est'], out['transformed_points'])
    stats = FuseLoss(cfg['loss'])(out, inp)
    assert torch.isfinite(stats['loss'])
    stats['loss'].backward()
    assert model.unet.conv_final.weight.grad is not None and model.motionhead.final_proj[0].weight.grad is None


def test_host_logic_no_foreground_gates(double):
    _no_foreground(double)


@pytest.mark.gpu
def test_gpu_no_foreground_gates():
    _no_foreground(torch.device('cuda:0'))


def test_dropin_import_paths():
    """the reference's import statements resolve to this package through dropin/."""
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'dropin'))
    try:
        for name in ('models', 'models.motionnet', 'models.pillar_encoder', 'models.cluster', 'libs', 'libs.voxel_generator',
                     'chamfer_distance', 'chamfer_distance.chamfer_distance'):
            sys.modules.pop(name, None)
        mn = importlib.import_module('models.motionnet')
        pe = importlib.import_module('models.pillar_encoder')
        vg = importlib.import_module('libs.voxel_generator')
        cd = importlib.import_module('chamfer_distance.chamfer_distance')
        assert mn.MotionNet is MotionNet
        assert all(hasattr(pe, n) for n in ('PillarFeatureNet', 'scatter_point_pillar', 'inverse_scatter_point_pillar', 'temporal_ungrid', 'ungrid'))
        assert hasattr(vg, 'Voxelization') and hasattr(cd, 'ChamferDistance')
        assert hasattr(importlib.import_module('models.cluster'), 'Cluster')
    finally:
        sys.path.remove(os.path.join(root, 'dropin'))
        for name in ('models', 'models.motionnet', 'models.pillar_encoder', 'models.cluster', 'libs', 'libs.voxel_generator',
                     'chamfer_distance', 'chamfer_distance.chamfer_distance'):
            sys.modules.pop(name, None)


@pytest.mark.gpu
@pytest.mark.parametrize('compute_dtype', ['fp32', 'bf16'])
def test_gpu_nuscene_geometry_train_step(compute_dtype):
    """nuScenes configuration (11 sweeps, configs/nuscene/nuscene.yaml) through the whole path: 3x3x3 stack over 11 frames, 10
    registration pairs per sample, both compute modes.  No golden vectors for this geometry: shapes and finiteness only."""
    dev = torch.device('cuda:0')
    cfg = default_config('nuscene', 'train', xy_range=12)
    cfg['misc']['compute_dtype'] = compute_dtype
    T = cfg['voxel_generator']['n_sweeps']
    # 3000 points per frame: with much sparser frames a registration pair can end up with no supported correspondence at all, and
    # the SVD of its zero covariance has no gradient -- in the reference too (its training loop skips such steps)
    inp = _to(make_batch(cfg, [3, 4], T, 3000), dev)
    torch.manual_seed(0)
    model = MotionNet(cfg)
    fill_state_dict_(model)
    model = model.to(dev).train()
    model.channels_last_()
    out = model(inp)
    stats = FuseLoss(cfg['loss'])(out, inp)
    stats['loss'].backward()
    assert out['ego_motion_est'].shape == (2, T, 4, 4) and out['fb_seg_est'].shape[:3] == (2, T, 2)
    assert out['rec_est'].shape == inp['input_points'].shape and torch.isfinite(out['rec_est']).all()
    assert torch.isfinite(stats['loss'].detach())
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.gpu
def test_gpu_device_sampler_flat_keypoint_gather():
    """Throughput configuration (pose_estimation.kpt_sampler = 'device'): gathering the key points of all pairs with five flat
    index ops gives what the per-pair loop gives for the same draws -- poses, permutation matrices, loss and the gradient
    reaching the ego feature head."""
    from helpers import oracle_voxeliser
    from pcaccumulation_amd.dataloader import collate_fn
    from pcaccumulation_amd.synthetic import make_sequence, attach_voxels
    cfg = default_config('waymo', 'train', n_sweeps=5, xy_range=8)
    cfg['pose_estimation']['kpt_sampler'] = 'device'
    vox = oracle_voxeliser(cfg)
    inp = collate_fn([attach_voxels(make_sequence(50, 5, 1500, cfg), vox), attach_voxels(make_sequence(51, 5, 900, cfg), vox)])
    dev = torch.device('cuda:0')
    outs = []
    for flat in (True, False):
        torch.manual_seed(5)
        model = MotionNet(cfg)
        fill_state_dict_(model)
        with torch.no_grad():
            model.semseg_head.seg_head[3].bias += torch.tensor([17.0, 0.0])
        model = model.to(dev).train()
        model.channels_last_()
        model.ego_motion_head.flat_keypoints = flat
        batch = _to(inp, dev)
        torch.manual_seed(6)
        out = model(batch)
        stats = FuseLoss(cfg['loss'])(out, batch)
        stats['loss'].backward()
        g = model.ego_feats_head.seg_head[0].weight.grad if hasattr(model.ego_feats_head, 'seg_head') else next(model.ego_feats_head.parameters()).grad
        outs.append((out['ego_motion_est'].detach().cpu(), torch.cat([p.detach() for p in out['perm_matrix']]).cpu(), float(stats['loss']), g.detach().cpu().clone()))
    (pose1, perm1, loss1, g1), (pose0, perm0, loss0, g0) = outs
    # same draws, same rows; the stacked operands are strided views in one case and fresh tensors in the other, so the batched
    # products may run in another order: fp32 rounding only
    assert (pose1 - pose0).abs().max() < 1e-4, (pose1 - pose0).abs().max()
    assert (perm1 - perm0).abs().max() < 1e-4, (perm1 - perm0).abs().max()
    assert abs(loss1 - loss0) <= 1e-4 * abs(loss0), (loss1, loss0)
    assert (g1 - g0).abs().max() <= 2e-2 * g0.abs().max(), ((g1 - g0).abs().max(), g0.abs().max())   # bf16 conv backward, atomic row sums


@pytest.mark.gpu
def test_gpu_library_conv_find_mode_is_the_same_step():
    """bench.py lets MIOpen pick the solver of the c_in >= 128 layers by measurement (torch.backends.cudnn.benchmark): same
    library, other kernels.  One bf16 train step with and without it: loss within 5e-3, U-Net bottleneck and head gradients
    pointing the same way (cosine > 0.98)."""
    from helpers import oracle_voxeliser
    from pcaccumulation_amd.dataloader import collate_fn
    from pcaccumulation_amd.synthetic import make_sequence, attach_voxels
    cfg = default_config('waymo', 'train', n_sweeps=3, xy_range=8)
    cfg['misc']['compute_dtype'] = 'bf16'
    vox = oracle_voxeliser(cfg)
    inp = collate_fn([attach_voxels(make_sequence(60, 3, 1500, cfg), vox), attach_voxels(make_sequence(61, 3, 1100, cfg), vox)])
    dev = torch.device('cuda:0')
    outs = []
    before = torch.backends.cudnn.benchmark
    try:
        for find in (False, True):
            torch.backends.cudnn.benchmark = find
            torch.manual_seed(5)
            model = MotionNet(cfg)
            fill_state_dict_(model)
            with torch.no_grad():
                model.semseg_head.seg_head[3].bias += torch.tensor([17.0, 0.0])
            model = model.to(dev).train()
            model.channels_last_()
            batch = _to(inp, dev)
            torch.manual_seed(6)
            out = model(batch)
            stats = FuseLoss(cfg['loss'])(out, batch)
            stats['loss'].backward()
            grads = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()
                     if p.grad is not None and p.dim() == 4 and (k.startswith('unet.down_convs.3') or k.startswith('semseg_head'))}   # conv weights (a bias in front of a BatchNorm has a zero gradient: rounding noise only)
            outs.append((float(stats['loss']), grads))
    finally:
        torch.backends.cudnn.benchmark = before
    (l0, g0), (l1, g1) = outs
    assert abs(l1 - l0) <= 5e-3 * abs(l0), (l0, l1)          # bf16 sums in another order flip a few arg-max / ReLU decisions
    assert g0 and set(g0) == set(g1)
    for k in g0:                                   # bf16 sums in another order, and a few ReLU / arg-max decisions downstream of them
        cos = torch.nn.functional.cosine_similarity(g1[k].reshape(-1), g0[k].reshape(-1), dim=0)
        assert cos > 0.98, (k, float(cos))


def _seq_pose(dev, golden, mode):
    """pose_estimation.seq_pose = chain / full (models/egomotion.py:195-307) on the tiny validation scene against the reference."""
    g, gs = golden('model_tiny_val'), golden('seqpose')
    cfg = default_config('waymo', 'val', n_sweeps=3, xy_range=8)
    cfg['pose_estimation']['seq_pose'] = mode
    model, inp = _build(g, cfg, dev, train=False)
    loss_fn = FuseLoss(cfg['loss'])
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
        stats = loss_fn(out, inp)
    c = lambda t: t.detach().float().cpu().numpy()
    np.testing.assert_allclose(c(out['ego_motion_est']), gs[mode + '_ego_motion_est'], atol=5e-3)
    np.testing.assert_allclose(c(out['ego_motion_gt']), gs[mode + '_ego_motion_gt'], atol=1e-5)
    assert abs(out['ego_rot_error'] - float(gs[mode + '_ego_rot_error'])) < 1e-3
    assert abs(out['ego_trans_error'] - float(gs[mode + '_ego_trans_error'])) < 1e-3
    assert abs(float(out['ego_l1_loss']) - float(gs[mode + '_ego_l1_loss'])) < 1e-3 * max(1.0, float(gs[mode + '_ego_l1_loss']))
    assert abs(float(out['ego_l2_loss']) - float(gs[mode + '_ego_l2_loss'])) < 1e-3 * max(1.0, float(gs[mode + '_ego_l2_loss']))
    assert len(out['perm_matrix']) == int(gs[mode + '_n_perm'])
    np.testing.assert_allclose(np.stack([c(p.sum(2)[0]) for p in out['perm_matrix']]), gs[mode + '_perm_rowsum'], atol=5e-3)
    assert abs(float(stats['perm_loss']) - float(gs[mode + '_perm_loss'])) < 1e-3 * max(1.0, abs(float(gs[mode + '_perm_loss'])))
    i, u = stats['mos_metric']['intersection'], stats['mos_metric']['union']
    assert abs(float((i / (u + 1e-20)).mean()) - float(gs[mode + '_mos_iou'])) < 1e-3


@pytest.mark.parametrize('mode', ['chain', 'full'])
def test_host_logic_seq_pose_modes(double, golden, mode):
    _seq_pose(double, golden, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['chain', 'full'])
def test_gpu_seq_pose_modes(golden, mode):
    _seq_pose(torch.device('cuda:0'), golden, mode)


def test_host_logic_duplicate_pillars_are_reported(double):
    """ops.PillarIndex(cell_order=True) needs one cell per pillar: a duplicated coordinate row is reported at the
    forward's host sync instead of turning into out-of-range gathers."""
    cfg = default_config('waymo', 'val', n_sweeps=3, xy_range=8)
    inp = make_batch(cfg, [5], 3, 600)
    inp['coordinates'][1] = inp['coordinates'][0]
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad(), pytest.raises(ValueError, match='occupied cells'):
        model.eval()(inp)
