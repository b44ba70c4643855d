"""The geometry kernels on a non-square grid with non-square cells.

Every kernel that turns metres into cells or back takes its x and y parameters separately (nx / ny, vx / vy, x_offset / y_offset,
x_scale / y_scale, x_reso / y_reso, x_min / y_min, h / w); on the square configurations of the other tests an exchanged pair computes the
same thing.  Here: range [-8,-6,-2,8,6,6], cells 0.25 x 0.125 m, nx = 64, ny = 96 (helpers.aniso_cfg), maps of 9 x 14 and 18 x 12 cells,
scales 8 and 6 -- no two members of a pair are equal.

Fixtures: tests/golden/aniso_ops.npz, written by tests/golden/make_golden_aniso.py from the reference itself.  Beside every fp32 output
of the reference it stores e = max |reference fp32 - the same formula in float64|, the reference's own distance from the truth; a
floating-point result passes within 4 x e (of the fixture on the CPU leg, of the float64 values on the GPU leg).  As printed by
`python tests/golden/make_golden.py aniso`:

    e_pillar_mean      4.768e-07      e_ungrid           1.763e-06      e_warp             3.955e-05
    e_pfn_out          7.948e-06      e_temporal_ungrid  2.435e-06      e_warp_small_c4    6.824e-06
    e_transformed      7.144e-07      e_gather_c4        2.533e-06      e_warp_small_c32   5.993e-06
                                      e_gather_c64       3.712e-06
    fb_margin (model_tiny_val_aniso, seeds 24 / 25)  9.014e-03, no flip on the CPU double; 22.2 % of the warped cells are exact zeros

CPU leg (not marked gpu): the numpy oracle, the C twin and the test double built on them (oracle/cpu_backend.py, through which the host-logic
tests run the model) against the fixture -- integers bit for bit -- which makes them a proven reference on this geometry.
GPU leg: every HIP entry point with an x / y pair against the fixture, the oracle or float64."""
import numpy as np
import pytest
import torch

import oracle
from oracle import cpu_backend, twin
from helpers import (ANISO_GEN_XY, ANISO_RANGE_OFF, ANISO_SMALL_WARP, aniso_batch, aniso_bev, aniso_cfg, aniso_gather_case, aniso_pillar_feats,
                     aniso_poses, aniso_warp_case, oracle_voxeliser, ungrid_f64, vox_points, warp_f64)
from pcaccumulation_amd.config import default_config

NX, NY, NT, B = 64, 96, 3, 2
X_SCALE, Y_SCALE = 8.0, 6.0
GATHER_SHAPE = (3, 9, 14)                    # n_maps, h, w of the synthetic gather case


@pytest.fixture(scope='module')
def fx(golden):
    return golden('aniso_ops')


@pytest.fixture(scope='module')
def batch(fx):
    """The collated two-sample batch of the fixture, voxelised by the oracle, with what several tests derive from it."""
    cfg, inp = aniso_batch([int(s) for s in fx['seeds']])
    pts = inp['input_points'].float().contiguous()
    p2v = inp['point_to_voxel_map'][:, 0].contiguous()
    assert int(p2v.min()) >= 0                                                         # every point has a pillar: no row is read through index -1
    m = inp['coordinates'].shape[0]
    mean = oracle.segment_mean(pts.numpy(), p2v.numpy().astype(np.int64), m)
    return dict(cfg=cfg, inp=inp, pts=pts, p2v=p2v, m=m, mean=mean)


@pytest.fixture(scope='module')
def warp64(fx):
    """float64 warp of the fixture's map (drawn again from its seed) and of its bf16 rounding: (bev, warped64, warped64 of the rounded map)."""
    bev, poses = aniso_bev(), fx['warp_poses']
    args = (0.25, 0.125, -8.0, -6.0)
    bev16 = torch.from_numpy(bev).to(torch.bfloat16).float().numpy()
    return bev, warp_f64(bev, poses, *args)[0], warp_f64(bev16, poses, *args)[0]


def _within(got, want, bound, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print('%s: max error %.3e, bound %.3e' % (what, err, bound))
    assert err <= bound, (what, err, bound)


def _cl(x):
    """[..., C, H, W] numpy -> contiguous channels-last torch tensor [..., H, W, C]."""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -3, -1)))


def _ref_cell(coords):
    c = np.asarray(coords).astype(np.int64)
    return ((c[:, 0] * NT + c[:, 4]) * NY + c[:, 2]) * NX + c[:, 3]


def _pfn_args(cfg):
    pe = cfg['pillar_encoder']
    vx, vy = pe['voxel_size'][0], pe['voxel_size'][1]
    return vx, vy, vx / 2 + pe['pc_range'][0], vy / 2 + pe['pc_range'][1], abs(pe['pc_range'][0]), pe['n_sweeps']


def _frame_index(inp):
    ti = inp['time_indice']
    return (ti[:, 0] * NT + ti[:, 1]).to(torch.int32)


# =========================================================================================================== CPU leg
@pytest.mark.parametrize('tag,pc_range', [('', None), ('off_', ANISO_RANGE_OFF)])
def test_oracle_voxelize_anisotropic(fx, tag, pc_range):
    cfg = aniso_cfg(pc_range=pc_range)
    vg = cfg['voxel_generator']
    pts = vox_points(1, 3000, cfg)
    assert oracle.grid_size(vg['voxel_size'], vg['range']).tolist() == [NX, NY, 1]
    out = oracle.voxelize(pts, vg['voxel_size'], vg['range'], vg['n_sweeps'])
    assert np.array_equal(out['shape'], fx['vox_%sshape' % tag]) and np.array_equal(out['num_voxels'], fx['vox_%snum_voxels' % tag])
    assert np.array_equal(out['coordinates'], fx['vox_%scoordinates' % tag])
    assert np.array_equal(out['point_to_voxel_map'], fx['vox_%sp2v' % tag])
    cap = oracle.voxelize(pts, vg['voxel_size'], vg['range'], vg['n_sweeps'], max_voxels=200)
    assert np.array_equal(cap['coordinates'], fx['vox_%scap_coordinates' % tag]) and np.array_equal(cap['point_to_voxel_map'], fx['vox_%scap_p2v' % tag])
    coords, p2v, num = cpu_backend.voxelize(torch.from_numpy(pts), vg['voxel_size'], vg['range'], [NX, NY, 1], NT, NX * NY * NT)
    assert int(num) == int(fx['vox_%snum_voxels' % tag][0]) and np.array_equal(coords[:int(num)].numpy(), fx['vox_%scoordinates' % tag])
    assert np.array_equal(p2v.numpy(), fx['vox_%sp2v' % tag][:, 0])


def test_oracle_batch_cells_and_pillar_features_anisotropic(fx, batch):
    """The collated batch is the reference's; cell index, pillar means, the nine pillar-encoder inputs and the encoder's output."""
    inp, pts, p2v, m, cfg = batch['inp'], batch['pts'], batch['p2v'], batch['m'], batch['cfg']
    assert np.array_equal(inp['coordinates'].numpy(), fx['coordinates']) and inp['coordinates'].dtype == torch.float64
    assert np.array_equal(inp['point_to_voxel_map'].numpy(), fx['p2v'])
    assert inp['shape'][0].tolist() == [NX, NY, 1, NT]
    want_cell = _ref_cell(fx['coordinates'])
    for coords in (inp['coordinates'], inp['coordinates'].to(torch.int32)):
        for cell, c2p in (twin.cell_index(coords.numpy(), NX, NY, NT, B), [t.numpy() for t in cpu_backend.cell_index(coords, NX, NY, NT, B)]):
            assert np.array_equal(cell, want_cell)
            assert c2p.shape == (B * NT * NY * NX,) and np.array_equal(c2p[want_cell], np.arange(m)) and int((c2p >= 0).sum()) == m
    _within(batch['mean'], fx['pillar_mean'], 4 * float(fx['e_pillar_mean']), 'pillar mean')
    pe = cfg['pillar_encoder']
    feats = oracle.pfn_features(pts.numpy(), p2v.numpy().astype(np.int64), inp['coordinates'].numpy(), fx['pillar_mean'], inp['time_indice'].numpy(),
                                pe['voxel_size'], pe['pc_range'], pe['n_sweeps'])
    for coords in (inp['coordinates'], inp['coordinates'].to(torch.int32)):
        got = cpu_backend.pfn_features(pts, p2v, torch.from_numpy(fx['pillar_mean']), coords, inp['time_indice'], *_pfn_args(cfg))
        assert np.array_equal(got.numpy(), feats)
    from pcaccumulation_amd.pillar_encoder import PillarFeatureNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    sd = {'pillar_encoder.' + k: v.numpy() for k, v in fill_state_dict_(PillarFeatureNet(pe)).state_dict().items()}
    out = oracle.pfn_forward(sd, feats, p2v.numpy().astype(np.int64), m, depth=pe['depth'])
    _within(out[::int(fx['pfn_stride'])], fx['pfn_out'], 4 * float(fx['e_pfn_out']), 'pillar encoder output')


def test_oracle_scatter_and_inverse_anisotropic(fx, batch):
    inp, m = batch['inp'], batch['m']
    feats = aniso_pillar_feats(m)
    shape = inp['shape'][0]
    assert np.array_equal(oracle.scatter_point_pillar(feats, fx['coordinates'], B, shape), fx['canvas'])
    cell, c2p = cpu_backend.cell_index(inp['coordinates'], NX, NY, NT, B)
    canvas = cpu_backend.pillar_scatter(torch.from_numpy(feats), c2p)
    assert np.array_equal(canvas.view(B, NT, NY, NX, 4).permute(0, 4, 1, 2, 3).numpy(), fx['canvas'])
    icanvas = fx['icanvas'].astype(np.int64)
    assert np.array_equal(oracle.inverse_scatter_point_pillar(icanvas, fx['coordinates'], B, shape), fx['inverse'])
    assert np.array_equal(cpu_backend.gather_rows(torch.from_numpy(icanvas.reshape(-1, 1)), cell).numpy(), fx['inverse'])


def test_oracle_ungrid_anisotropic(fx):
    pts, ti = fx['ungrid_points'], fx['ungrid_time_indice']
    rng = [-X_SCALE, -Y_SCALE, -2, X_SCALE, Y_SCALE, 6]
    b4, bt = 4 * float(fx['e_ungrid']), 4 * float(fx['e_temporal_ungrid'])
    assert 0.1 < float((np.abs(pts[:, 0]) > X_SCALE).mean()) < 0.25 and 0.1 < float((np.abs(pts[:, 1]) > Y_SCALE).mean()) < 0.25   # a sixth beyond the map on each axis
    _within(oracle.ungrid(fx['ungrid_fmap'], pts, rng, ti), fx['ungrid_out'], b4, 'oracle.ungrid')
    _within(oracle.temporal_ungrid(fx['ungrid_fmap_t'], pts, rng, ti), fx['ungrid_out_t'], bt, 'oracle.temporal_ungrid')
    before = pts.copy()
    got = cpu_backend.bilinear_gather(_cl(fx['ungrid_fmap']), torch.from_numpy(pts), torch.from_numpy(ti[:, 0].astype(np.int32)), X_SCALE, Y_SCALE)
    _within(got.numpy(), fx['ungrid_out'], b4, 'double bilinear_gather')
    tidx = torch.from_numpy((ti[:, 0] * NT + ti[:, 1]).astype(np.int32))
    got = cpu_backend.bilinear_gather(_cl(fx['ungrid_fmap_t']).reshape(B * NT, 9, 14, 4), torch.from_numpy(pts), tidx, X_SCALE, Y_SCALE)
    _within(got.numpy(), fx['ungrid_out_t'], bt, 'double bilinear_gather, temporal')
    assert np.array_equal(pts, before)
    # the backward of the double (float32 autograd of grid_sample) against the float64 gradient on the synthetic case
    fm, sp, si, go = aniso_gather_case(4)
    g = cpu_backend.bilinear_gather_backward(torch.from_numpy(go), fm.shape, torch.from_numpy(sp), torch.from_numpy(si), X_SCALE, Y_SCALE)
    np.testing.assert_allclose(g.numpy(), _gather_grad_f64(fm.shape, sp, si, go), rtol=1e-4, atol=1e-4)


def test_oracle_warp_and_transform_anisotropic(fx, batch):
    bev, poses = aniso_bev(), fx['warp_poses']
    assert np.array_equal(poses, aniso_poses())
    bound = 4 * float(fx['e_warp'])
    want = oracle.warp_feats(bev, poses, [0.25, 0.125, 8], [-8, -6, -2, 8, 6, 6])
    _within(want[:, 1:], fx['warped'], bound, 'oracle.warp_feats')
    assert np.array_equal(want[:, 0], bev[:, -1])
    inv = torch.linalg.inv(torch.from_numpy(poses)).contiguous()
    got = cpu_backend.bev_warp(_cl(bev), inv, 0.25, 0.125, -8.0, -6.0).permute(0, 1, 4, 2, 3).numpy()
    _within(got[:, 1:], fx['warped'], bound, 'double bev_warp')
    assert np.array_equal(got[:, 0], bev[:, -1])
    inp, pts = batch['inp'], batch['pts']
    stride, bound = int(fx['tp_stride']), 4 * float(fx['e_transformed'])
    _within(oracle.transform_points(pts.numpy(), inp['time_indice'].numpy(), poses)[::stride], fx['transformed'], bound, 'oracle.transform_points')
    tp = cpu_backend.rigid_transform(pts, _frame_index(inp), torch.from_numpy(poses).reshape(-1, 16))
    _within(tp.numpy()[::stride], fx['transformed'], bound, 'double rigid_transform')


def _gather_grad_f64(shape, pts, idx, go):
    """float64 autograd gradient of grid_sample(border) w.r.t. a [n,h,w,c] map; points of no map contribute nothing."""
    n, h, w, c = shape
    f = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
    p, g = torch.from_numpy(np.asarray(pts, np.float64)), torch.from_numpy(np.asarray(go, np.float64))
    tot = 0
    for b in range(n):
        sel = torch.from_numpy(np.asarray(idx) == b)
        if bool(sel.any()):
            grid = torch.stack([p[sel, 0] / X_SCALE, p[sel, 1] / Y_SCALE], 1).view(1, -1, 1, 2)
            s = torch.nn.functional.grid_sample(f[b:b + 1], grid, mode='bilinear', padding_mode='border', align_corners=False)
            tot = tot + (s[0, :, :, 0].T * g[sel]).sum()
    tot.backward()
    return f.grad.permute(0, 2, 3, 1).numpy()


# =========================================================================================================== GPU leg
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def native():
    from pcaccumulation_amd import native as n
    n.lib()
    return n


@pytest.fixture(scope='module')
def index(native, dev, batch):
    cell, c2p = native.cell_index(batch['inp']['coordinates'].to(dev), NX, NY, NT, B)
    return cell, c2p


@pytest.mark.gpu
@pytest.mark.parametrize('tag,pc_range', [('', None), ('off_', ANISO_RANGE_OFF)])
def test_voxelize_anisotropic(native, dev, fx, tag, pc_range):
    cfg = aniso_cfg(pc_range=pc_range)
    vg = cfg['voxel_generator']
    pts = torch.from_numpy(vox_points(1, 3000, cfg)).to(dev)
    grid = oracle.grid_size(vg['voxel_size'], vg['range'])
    for mv, ck, pk in ((NX * NY * NT, 'vox_%scoordinates', 'vox_%sp2v'), (200, 'vox_%scap_coordinates', 'vox_%scap_p2v')):
        coords, p2v, num = native.voxelize(pts, vg['voxel_size'], vg['range'], grid, NT, mv)
        m = int(num.item())
        assert m == min(mv, int(fx['vox_%snum_voxels' % tag][0]))
        assert np.array_equal(coords[:m].cpu().numpy(), fx[ck % tag])
        assert np.array_equal(p2v.cpu().numpy(), fx[pk % tag][:, 0])


@pytest.mark.gpu
def test_collate_voxelize_anisotropic(native, dev, fx, monkeypatch):
    """pcacc_collate_voxelize on the anisotropic grid == per-sample voxelisation by the oracle + collate_fn, and == the per-sample launches.  Sample 1
    has points with 6 < |y| < 8 (inside a grid whose extents were exchanged, outside this one) and with 6 < |x| < 8 (the other way round)."""
    from pcaccumulation_amd.dataloader import collate_fn
    from pcaccumulation_amd.pipeline import DeviceBatcher, sample_to_device
    from pcaccumulation_amd.synthetic import make_sequence, attach_voxels
    cfg = aniso_cfg('train')
    gen_cfg = default_config('waymo', 'train', n_sweeps=NT, xy_range=ANISO_GEN_XY)
    raw = [make_sequence(int(s), NT, n, gen_cfg) for s, n in zip(fx['seeds'], (1500, 900))]
    raw[1]['input_points'][::7, 1] += 7.0
    raw[1]['input_points'][3::7, 0] += 2.0
    raw[1]['time_indice'][::11, 0] = 5
    want = collate_fn([attach_voxels(dict(r), oracle_voxeliser(cfg)) for r in raw])
    y, x = raw[1]['input_points'][:, 1], raw[1]['input_points'][:, 0]
    assert ((np.abs(y) > 6) & (np.abs(y) < 8)).sum() > 50 and ((np.abs(x) > 6) & (np.abs(x) < 8)).sum() > 50
    samples = [sample_to_device(r, dev) for r in raw]
    got = DeviceBatcher(cfg)(samples)
    monkeypatch.setenv('PCACC_BATCHED_COLLATE', '0')
    old = DeviceBatcher(cfg)(samples)
    for name, other in (('reference layout', want), ('per-sample path', old)):
        for k, v in other.items():
            if k == 'inst_motion_gt':
                assert all(torch.equal(a.cpu(), torch.as_tensor(b).cpu()) for a, b in zip(got[k], v)), (name, k)
                continue
            v = torch.as_tensor(v)
            assert got[k].dtype == v.dtype and tuple(got[k].shape) == tuple(v.shape), (name, k, got[k].dtype, v.dtype, got[k].shape, v.shape)
            assert torch.equal(got[k].cpu(), v.cpu()), (name, k)


@pytest.mark.gpu
def test_cell_index_and_frame_pillars_anisotropic(native, dev, batch):
    coords = batch['inp']['coordinates']
    m = batch['m']
    cell, c2p = native.cell_index(coords.to(dev), NX, NY, NT, B)
    ref_cell = _ref_cell(coords.numpy())
    assert np.array_equal(cell.cpu().numpy(), ref_cell)
    ref_c2p = np.full(B * NT * NY * NX, -1, np.int64)
    ref_c2p[ref_cell] = np.arange(m)
    assert np.array_equal(c2p.cpu().numpy(), ref_c2p)
    cell_i, c2p_i = native.cell_index(coords.to(torch.int32).to(dev), NX, NY, NT, B)
    assert torch.equal(cell_i, cell) and torch.equal(c2p_i, c2p)
    sp, offs = native.frame_pillars(c2p, NY * NX, m)
    occ = ref_c2p >= 0
    assert np.array_equal(sp.cpu().numpy(), ref_c2p[occ])
    assert np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum(occ.reshape(-1, NY * NX).sum(1))]))


@pytest.mark.gpu
def test_pfn_features_and_encoder_anisotropic(native, dev, fx, batch):
    """pcacc_pfn_features bit for bit against the oracle (f64 and i32 coordinates), pcacc_pfn_features_ordered == its rows in the order of a real CSR,
    and the whole pillar encoder against the reference's output."""
    from pcaccumulation_amd import ops
    from pcaccumulation_amd.pillar_encoder import PillarFeatureNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    inp, pts, p2v, m, cfg = batch['inp'], batch['pts'], batch['p2v'], batch['m'], batch['cfg']
    pe = cfg['pillar_encoder']
    mean = batch['mean']
    ref = oracle.pfn_features(pts.numpy(), p2v.numpy().astype(np.int64), inp['coordinates'].numpy(), mean, inp['time_indice'].numpy(),
                              pe['voxel_size'], pe['pc_range'], pe['n_sweeps'])
    args = (pts.to(dev), p2v.to(dev), torch.from_numpy(mean).to(dev))
    ti = inp['time_indice'].to(dev)
    got = native.pfn_features(*args, inp['coordinates'].to(dev), ti, *_pfn_args(cfg))
    assert np.array_equal(got.cpu().numpy(), ref)
    got_i = native.pfn_features(*args, inp['coordinates'].to(torch.int32).to(dev), ti, *_pfn_args(cfg))
    assert torch.equal(got_i, got)
    offs, order = native.csr_build(p2v.to(dev), m)
    assert np.array_equal(order.cpu().numpy(), np.argsort(p2v.numpy(), kind='stable'))
    got_o = native.pfn_features(*args, inp['coordinates'].to(dev), ti, *_pfn_args(cfg), order=order)
    assert torch.equal(got_o, got[order.long()])
    pfn = fill_state_dict_(PillarFeatureNet(pe)).to(dev).eval()
    pidx = ops.PillarIndex(inp['coordinates'].to(dev), inp['point_to_voxel_map'].to(dev), B, [int(v) for v in inp['shape'][0]])
    with torch.no_grad():
        out = pfn(pts.to(dev), None, inp['coordinates'].to(dev), torch.from_numpy(mean).to(dev), ti, pidx=pidx)
    np.testing.assert_allclose(out.cpu().numpy()[::int(fx['pfn_stride'])], fx['pfn_out'], rtol=1e-4, atol=5e-5)


@pytest.mark.gpu
def test_pillar_scatter_and_gather_anisotropic(native, dev, fx, batch, index):
    cell, c2p = index
    feats = torch.from_numpy(aniso_pillar_feats(batch['m'])).to(dev)
    canvas = native.pillar_scatter(feats, c2p)
    got = canvas.view(B, NT, NY, NX, 4).permute(0, 4, 1, 2, 3)
    assert np.array_equal(got.cpu().numpy(), fx['canvas'])
    c16 = native.pillar_scatter(feats, c2p, torch.bfloat16)
    assert c16.dtype == torch.bfloat16
    assert torch.equal(c16.view(B, NT, NY, NX, 4).permute(0, 4, 1, 2, 3).cpu(), torch.from_numpy(fx['canvas']).to(torch.bfloat16))
    ic = torch.from_numpy(fx['icanvas'].astype(np.int64)).reshape(-1, 1).contiguous()
    assert np.array_equal(native.gather_rows(ic.to(dev), cell).cpu().numpy(), fx['inverse'])
    assert torch.equal(native.gather_rows(canvas, cell), feats)


@pytest.mark.gpu
def test_pooling_into_the_canvas_anisotropic(native, dev, batch, index):
    """pcacc_segment_max_canvas == pcacc_segment_max followed by pcacc_pillar_scatter, forward and backward, on the anisotropic batch."""
    cell, c2p = index
    p2v, m = batch['p2v'].to(dev), batch['m']
    n = p2v.shape[0]
    rng = np.random.RandomState(5)
    src = rng.randn(n, 32).astype(np.float32)
    src[rng.randint(0, n, 500)] = src[rng.randint(0, n, 500)]                          # exact ties across points
    src = torch.from_numpy(src).to(dev)
    offs, order = native.csr_build(p2v, m)
    pooled, arg = native.segment_max(src, offs, order, m)
    want32 = native.pillar_scatter(pooled, c2p)
    want16 = native.pillar_scatter(pooled.to(torch.bfloat16), c2p, torch.bfloat16)
    got32, got16, got_arg = native.segment_max_canvas(src, offs, order, m, c2p)
    assert torch.equal(got32, want32) and torch.equal(got16, want16) and torch.equal(got_arg, arg)
    assert float(got32[c2p < 0].abs().max()) == 0.0
    # pinned to the reference's layout, not only to the other kernel: cell (b, t, y, x) of the canvas holds the pooled row of the pillar there
    c = batch['inp']['coordinates'].long().to(dev)
    assert torch.equal(got32.view(B, NT, NY, NX, 32)[c[:, 0], c[:, 4], c[:, 2], c[:, 3]], pooled)
    for dt in (torch.bfloat16, torch.float32):
        g = torch.from_numpy(rng.randn(c2p.numel(), 32).astype(np.float32)).to(dev).to(dt)
        want = native.segment_max_backward(native.gather_rows(g, cell), arg, p2v, n, out_dtype=torch.bfloat16)
        assert torch.equal(native.segment_max_canvas_backward(g, arg, p2v, cell, n, out_dtype=torch.bfloat16), want)


@pytest.mark.gpu
def test_bilinear_gather_fixture_anisotropic(native, dev, fx):
    """ungrid and temporal_ungrid on 9 x 14 maps with scales 8 and 6: within 4 x e of float64 -- fp32 map, and bf16 map against float64 sampling of
    the rounded map (the rounding is in the input, the arithmetic is the same)."""
    pts_np, ti = fx['ungrid_points'], fx['ungrid_time_indice']
    pts = torch.from_numpy(pts_np).to(dev)
    bidx = ti[:, 0].astype(np.int32)
    tidx = (ti[:, 0] * NT + ti[:, 1]).astype(np.int32)
    fm, fm_t = fx['ungrid_fmap'], fx['ungrid_fmap_t'].reshape(B * NT, 4, 9, 14)
    for name, maps, idx, e in (('ungrid', fm, bidx, fx['e_ungrid']), ('temporal_ungrid', fm_t, tidx, fx['e_temporal_ungrid'])):
        cl = _cl(maps)
        out = native.bilinear_gather(cl.to(dev), pts, torch.from_numpy(idx).to(dev), X_SCALE, Y_SCALE)
        _within(out.cpu().numpy(), ungrid_f64(maps, pts_np, idx, X_SCALE, Y_SCALE), 4 * float(e), name + ' f32')
        cl16 = cl.to(torch.bfloat16)
        out = native.bilinear_gather(cl16.to(dev), pts, torch.from_numpy(idx).to(dev), X_SCALE, Y_SCALE)
        assert out.dtype == torch.float32
        _within(out.cpu().numpy(), ungrid_f64(cl16.float().permute(0, 3, 1, 2).numpy(), pts_np, idx, X_SCALE, Y_SCALE), 4 * float(e), name + ' bf16')
    assert torch.equal(pts.cpu(), torch.from_numpy(pts_np))


@pytest.fixture(scope='module', params=[4, 64])
def gcase(request, fx):
    """The synthetic gather case for c channels with its float64 forward values and map gradient, computed once."""
    c = request.param
    fm, pts, idx, go = aniso_gather_case(c)
    assert fm.shape[:3] == GATHER_SHAPE and pts.shape[0] == 700 and int((idx == -1).sum()) == 10 and int((idx == 3).sum()) == 10
    fwd = ungrid_f64(fm.transpose(0, 3, 1, 2), pts, idx, X_SCALE, Y_SCALE)
    return dict(c=c, fm=fm, pts=pts, idx=idx, go=go, fwd=fwd, grad=_gather_grad_f64(fm.shape, pts, idx, go), e=float(fx['e_gather_c%d' % c]))


@pytest.mark.gpu
def test_bilinear_gather_synthetic_anisotropic(native, dev, gcase):
    g = gcase
    pts = torch.from_numpy(g['pts']).to(dev)
    out = native.bilinear_gather(torch.from_numpy(g['fm']).to(dev), pts, torch.from_numpy(g['idx']).to(dev), X_SCALE, Y_SCALE).cpu().numpy()
    bad = (g['idx'] < 0) | (g['idx'] >= GATHER_SHAPE[0])
    assert int(bad.sum()) == 20 and not out[bad].any()
    _within(out, g['fwd'], 4 * g['e'], 'bilinear_gather c=%d' % g['c'])
    assert torch.equal(pts.cpu(), torch.from_numpy(g['pts']))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int16))


@pytest.mark.gpu
def test_bilinear_backward_anisotropic(native, dev, gcase):
    """Map gradient of the gather at h = 9, w = 14 (the sorted kernel's 4 x 4 tiles are ragged on both axes, with remainders 1 and 2), scales 8 and 6: the
    atomic kernel, the sorted kernel and ops.bilinear_gather(...).backward against the float64 autograd gradient of grid_sample(border) at the bound of
    test_bilinear_gather_backward_vs_autograd; rows of no map contribute nothing; bf16 in / bf16 out at the bound of
    test_bilinear_gather_backward_sorted_matches_atomic."""
    from pcaccumulation_amd import ops
    g = gcase
    shape = g['fm'].shape
    pts, idx, go = torch.from_numpy(g['pts']).to(dev), torch.from_numpy(g['idx']).to(dev), torch.from_numpy(g['go']).to(dev)
    atomic = native.bilinear_gather_backward(go, shape, pts, idx, X_SCALE, Y_SCALE)
    np.testing.assert_allclose(atomic.cpu().numpy(), g['grad'], rtol=1e-4, atol=1e-4)
    srt = native.bilinear_gather_backward_sorted(go, shape, pts, idx, X_SCALE, Y_SCALE)
    assert srt.dtype == torch.float32
    np.testing.assert_allclose(srt.cpu().numpy(), g['grad'], rtol=1e-4, atol=1e-4)
    base = torch.from_numpy(g['fm']).to(dev).requires_grad_(True)                      # [n,h,w,c] storage behind a logical [n,c,h,w] map
    out = ops.bilinear_gather(base.permute(0, 3, 1, 2), pts, idx, X_SCALE, Y_SCALE)
    out.backward(go)
    np.testing.assert_allclose(base.grad.cpu().numpy(), g['grad'], rtol=1e-4, atol=1e-4)
    # rows of no map: the same sums, in the same order, as without them -- whatever their gradient holds
    keep = torch.from_numpy((g['idx'] >= 0) & (g['idx'] < shape[0])).to(dev)
    loud = go.clone()
    loud[~keep] = 1e30
    assert _bits_equal(native.bilinear_gather_backward_sorted(loud, shape, pts, idx, X_SCALE, Y_SCALE), srt)
    assert _bits_equal(native.bilinear_gather_backward_sorted(go[keep], shape, pts[keep], idx[keep], X_SCALE, Y_SCALE), srt)
    np.testing.assert_allclose(native.bilinear_gather_backward(loud, shape, pts, idx, X_SCALE, Y_SCALE).cpu().numpy(), g['grad'], rtol=1e-4, atol=1e-4)
    go16 = go.to(torch.bfloat16)
    got16 = native.bilinear_gather_backward_sorted(go16, shape, pts, idx, X_SCALE, Y_SCALE, out_dtype=torch.bfloat16)
    ref16 = native.bilinear_gather_backward_sorted(go16.float(), shape, pts, idx, X_SCALE, Y_SCALE)
    assert got16.dtype == torch.bfloat16 and (got16.float() - ref16).abs().max().item() <= 2 ** -7 * max(1.0, ref16.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('c', [4, 64])
def test_bilinear_backward_crowded_cells_anisotropic(native, dev, c):
    """More than BG_CROWD = 8 points in one cell go through the sorted kernel's work list.  Three such cells on the 9 x 14 map, one per map: 40 points
    inside base cell (x = w-2, y = h-2) (four taps, the last row and column among them), 40 clamped onto the far corner (w-1, h-1) (one tap, no
    neighbour), 40 inside base cell (0, 0); among them the 700 points of the synthetic case."""
    n_maps, h, w = GATHER_SHAPE
    fm, pts, idx, go = aniso_gather_case(c)
    rng = np.random.RandomState(300 + c)

    def metres(px, py):                                                                 # pixel coordinates (align_corners=False) -> metres
        return np.stack([((px + 0.5) * 2.0 / w - 1.0) * X_SCALE, ((py + 0.5) * 2.0 / h - 1.0) * Y_SCALE, np.zeros_like(px)], 1)
    f = rng.uniform(0.1, 0.9, (3, 2, 40))
    extra = np.concatenate([metres(w - 2 + f[0, 0], h - 2 + f[0, 1]), metres(w + 3 * f[1, 0], h + 3 * f[1, 1]), metres(f[2, 0], f[2, 1])]).astype(np.float32)
    pts = np.concatenate([pts, extra])
    idx = np.concatenate([idx, np.repeat(np.arange(3, dtype=np.int32), 40)])
    go = np.concatenate([go, rng.randn(120, c).astype(np.float32)])
    perm = rng.permutation(pts.shape[0])                                                # the points of a cell are not neighbours in memory
    pts, idx, go = pts[perm], idx[perm], go[perm]
    shape = (n_maps, h, w, c)
    want = _gather_grad_f64(shape, pts, idx, go)
    tp, ti, tg = torch.from_numpy(pts).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(go).to(dev)
    valid = (idx >= 0) & (idx < n_maps)                                                 # base cell of every point, as make_taps<BORDER> finds it
    bx = np.floor(np.clip(((pts[:, 0].astype(np.float64) / X_SCALE + 1) * w - 1) / 2, 0, w - 1)).astype(np.int64)
    by = np.floor(np.clip(((pts[:, 1].astype(np.float64) / Y_SCALE + 1) * h - 1) / 2, 0, h - 1)).astype(np.int64)
    count = np.bincount(np.where(valid, (idx.astype(np.int64) * h + by) * w + bx, n_maps * h * w), minlength=n_maps * h * w + 1)
    for mi, y, x in ((0, h - 2, w - 2), (1, h - 1, w - 1), (2, 0, 0)):                  # the three cells are crowded, and nothing needs the > 64 path
        assert count[(mi * h + y) * w + x] >= 40
    assert count[:-1].max() <= 64 and count[-1] == 20
    got = native.bilinear_gather_backward_sorted(tg, shape, tp, ti, X_SCALE, Y_SCALE)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4)
    assert _bits_equal(native.bilinear_gather_backward_sorted(tg, shape, tp, ti, X_SCALE, Y_SCALE), got)
    np.testing.assert_allclose(native.bilinear_gather_backward(tg, shape, tp, ti, X_SCALE, Y_SCALE).cpu().numpy(), want, rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_bev_warp_fixture_anisotropic(native, dev, fx, warp64):
    """warp_feats on the 96 x 64 map (cells 0.25 x 0.125 m): fp32 within 4 x e_warp of float64, slot 0 = the last frame bit for bit; bf16 map within the
    same bound plus 2^-8 |value| (the one rounding on store) of the float64 warp of the rounded map; the reference's own fp32 result as well."""
    bev, w64, w64_16 = warp64
    inv = torch.linalg.inv(torch.from_numpy(fx['warp_poses'])).contiguous().to(dev)
    bound = 4 * float(fx['e_warp'])
    cl = _cl(bev)
    got = native.bev_warp(cl.to(dev), inv, 0.25, 0.125, -8.0, -6.0).permute(0, 1, 4, 2, 3).cpu().numpy()
    _within(got, w64, bound, 'bev_warp f32')
    _within(got[:, 1:], fx['warped'], 2 * bound, 'bev_warp f32 against the reference')          # each within 4 e of the truth
    assert np.array_equal(got[:, 0], bev[:, -1])
    cl16 = cl.to(torch.bfloat16)
    got16 = native.bev_warp(cl16.to(dev), inv, 0.25, 0.125, -8.0, -6.0)
    assert got16.dtype == torch.bfloat16
    got16 = got16.float().permute(0, 1, 4, 2, 3).cpu().numpy().astype(np.float64)
    excess = np.abs(got16 - w64_16) - 2.0 ** -8 * np.abs(w64_16)
    print('bev_warp bf16: max error beyond 2^-8 |value| %.3e, bound %.3e' % (float(excess.max()), bound))
    assert float(excess.max()) <= bound
    assert torch.equal(torch.from_numpy(got16[:, 0]).float(), cl16.float().permute(0, 1, 4, 2, 3)[:, -1])


@pytest.fixture(scope='module', params=[4, 32])
def wcase(request, fx):
    c = request.param
    bev, poses = aniso_warp_case(c)
    w64, px, py = warp_f64(bev, poses, *ANISO_SMALL_WARP)
    zero = np.abs(w64[:, 1:]).max(2) == 0                                              # [B,T-1,H,W]
    # a condition on the inputs, not on the kernel: the poses move a good part of every frame out of the map, and leave a good part inside
    assert 0.10 <= float(zero.mean()) <= 0.50, float(zero.mean())
    return dict(c=c, bev=bev, poses=poses, w64=w64, px=px, py=py, zero=zero, e=float(fx['e_warp_small_c%d' % c]))


@pytest.mark.gpu
def test_bev_warp_synthetic_anisotropic(native, dev, wcase):
    """18 x 12 map over 16 m x 12 m (x_reso = 4/3, y_reso = 2/3), rotations of +-0.3 and +-1.5 rad: within 4 x e of float64; a cell that is zero in
    float64 and samples more than one pixel outside the map is exactly zero."""
    k = wcase
    h, w = 18, 12
    inv = torch.linalg.inv(torch.from_numpy(k['poses'])).contiguous().to(dev)
    got = native.bev_warp(_cl(k['bev']).to(dev), inv, *ANISO_SMALL_WARP).permute(0, 1, 4, 2, 3).cpu().numpy()
    _within(got, k['w64'], 4 * k['e'], 'bev_warp 18 x 12, c=%d' % k['c'])
    assert np.array_equal(got[:, 0], k['bev'][:, -1])
    px, py = k['px'][:, 1:], k['py'][:, 1:]
    far = k['zero'] & ((px < -2) | (px > w + 1) | (py < -2) | (py > h + 1))            # taps at floor(p), floor(p) + 1: none inside below -1 / from size on
    assert far.sum() > 0.05 * far.size
    assert not np.abs(got[:, 1:]).max(2)[far].any()


@pytest.mark.gpu
def test_bev_warp_non_finite_pose_anisotropic(native, dev, wcase):
    """make_taps: 'NaN / huge coordinates: every validity test fails, the sample is zero'.  One frame's inverse pose all NaN, another's all +inf: those two
    output frames are exactly zero, every other frame is bit-identical to the run with finite poses."""
    k = wcase
    bev = _cl(k['bev']).to(dev)
    inv = torch.linalg.inv(torch.from_numpy(k['poses'])).contiguous()
    want = native.bev_warp(bev, inv.to(dev), *ANISO_SMALL_WARP)
    bad = inv.clone()
    bad[0, 1] = float('nan')
    bad[1, 2] = float('inf')
    got = native.bev_warp(bev, bad.to(dev), *ANISO_SMALL_WARP)
    assert not got[0, 1].any() and not got[1, 2].any()
    assert bool(torch.isfinite(got).all())
    for b, t in ((0, 0), (0, 2), (1, 0), (1, 1)):
        assert _bits_equal(got[b, t], want[b, t]), (b, t)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['fixture', 'small'])
def test_bev_warp_dual_anisotropic(native, dev, fx, shape):
    """pcacc_bev_warp_dual: the fp32 result bit-identical to pcacc_bev_warp, the second output its bf16 rounding; ops.bev_warp_enter_mixed in the
    'mixed' mode returns that pair (the bf16 shadow, registered with the fp32 result as its twin)."""
    from pcaccumulation_amd import ops
    if shape == 'fixture':
        bev, poses, args = aniso_bev(), fx['warp_poses'], (0.25, 0.125, -8.0, -6.0)
    else:
        (bev, poses), args = aniso_warp_case(32), ANISO_SMALL_WARP
    cl = _cl(bev).to(dev)
    inv = torch.linalg.inv(torch.from_numpy(poses)).contiguous().to(dev)
    want = native.bev_warp(cl, inv, *args)
    out, out16 = native.bev_warp_dual(cl, inv, *args)
    assert out.dtype == torch.float32 and out16.dtype == torch.bfloat16 and out16.shape == out.shape
    assert _bits_equal(out, want)
    assert _bits_equal(out16, out.to(torch.bfloat16))
    ops.set_mixed(True)
    try:
        r = ops.bev_warp_enter_mixed(cl, inv, *args)
        assert r.dtype == torch.bfloat16 and _bits_equal(r, out16)
        assert _bits_equal(ops.twin(r), want)
    finally:
        ops.set_mixed(False)
    plain = ops.bev_warp_enter_mixed(cl, inv, *args)                                   # outside the mixed mode: the fp32 warp itself
    assert plain.dtype == torch.float32 and _bits_equal(plain, want)


@pytest.mark.gpu
def test_rigid_transform_anisotropic(native, dev, fx, batch):
    inp = batch['inp']
    tp = native.rigid_transform(batch['pts'].to(dev), _frame_index(inp).to(dev), torch.from_numpy(fx['warp_poses']).reshape(-1, 16).contiguous().to(dev))
    _within(tp.cpu().numpy()[::int(fx['tp_stride'])], fx['transformed'], 4 * float(fx['e_transformed']), 'rigid_transform')
