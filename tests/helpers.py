"""Shared builders for the parity tests (inputs are regenerated from seeds, never read from /root/reference)."""
import os
import shutil
import subprocess

import numpy as np

import oracle
from pcaccumulation_amd.config import default_config, update_config
from pcaccumulation_amd.dataloader import collate_fn
from pcaccumulation_amd.synthetic import make_sequence, attach_voxels


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_driver(tmp_path, name):
    """g++ build of tests/<name>.cpp on the headers of pcaccumulation_amd/csrc -- the code the kernels run -- without FMA contraction and with every
    table index assert-checked (csrc/hd.h: PCACC_BOUND); returns the executable in tmp_path."""
    exe = os.path.join(str(tmp_path), name)
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'the host-build test needs a C++ compiler'
    subprocess.check_call([cxx, '-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DPCACC_HOST_CHECK', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'pcaccumulation_amd', 'csrc'), os.path.join(ROOT, 'tests', name + '.cpp'), '-o', exe])
    return exe


def oracle_voxeliser(cfg):
    vg = cfg['voxel_generator']

    def f(points):
        out = oracle.voxelize(points, vg['voxel_size'], vg['range'], vg['n_sweeps'])
        out.pop('num_points_per_voxel')
        return out
    return f


def small_cfg(mode='val'):
    return default_config('waymo', mode, n_sweeps=3, xy_range=8)


ANISO_RANGE = [-8, -6, -2, 8, 6, 6]          # 16 m x 12 m: |x_min| = 8 and |y_min| = 6 differ
ANISO_RANGE_OFF = [-8, -3, -2, 8, 9, 6]       # same extent, not centred in y
ANISO_VOXEL = [0.25, 0.125, 8]                # nx = 64, ny = 96: every x / y pair of the geometry kernels differs
ANISO_GEN_XY = 6                              # sequences are drawn for this half-extent, so that every point has a pillar


def aniso_cfg(mode='val', pc_range=None):
    """Non-square grid with non-square cells, 3 sweeps (tests/golden/make_golden_aniso.py builds its fixtures on it)."""
    cfg = default_config('waymo', mode, n_sweeps=3, xy_range=ANISO_GEN_XY)
    cfg['voxel_generator']['range'] = list(pc_range or ANISO_RANGE)
    cfg['voxel_generator']['voxel_size'] = list(ANISO_VOXEL)
    return update_config(cfg)


def aniso_batch(seeds, n_frames=3, pts_per_frame=1500, mode='val', voxeliser=None):
    """Sequences drawn on the square extent ANISO_GEN_XY (make_sequence only knows square ones), voxelised on the anisotropic grid."""
    cfg = aniso_cfg(mode)
    gen_cfg = default_config('waymo', mode, n_sweeps=n_frames, xy_range=ANISO_GEN_XY)
    vox = voxeliser or oracle_voxeliser(cfg)
    return cfg, collate_fn([attach_voxels(make_sequence(int(s), n_frames, pts_per_frame, gen_cfg), vox) for s in seeds])


def ungrid_f64(fmap, points, map_idx, x_scale, y_scale):
    """float64 statement of ungrid / temporal_ungrid: grid_sample(bilinear, border, align_corners=False) on double tensors.  fmap [n_maps,C,H,W],
    points [K,>=2], map_idx [K]; rows whose map index lies outside [0, n_maps) are zero.  -> [K,C] float64."""
    import torch
    f = torch.from_numpy(np.ascontiguousarray(fmap, np.float64))
    p = np.asarray(points, np.float64)
    idx = np.asarray(map_idx).astype(np.int64)
    out = np.zeros((p.shape[0], f.shape[1]), np.float64)
    for b in range(f.shape[0]):
        sel = np.nonzero(idx == b)[0]
        if sel.size:
            grid = torch.from_numpy(np.stack([p[sel, 0] / x_scale, p[sel, 1] / y_scale], 1)).view(1, -1, 1, 2)
            s = torch.nn.functional.grid_sample(f[b:b + 1], grid, mode='bilinear', padding_mode='border', align_corners=False)
            out[sel] = s[0, :, :, 0].T.numpy()
    return out


def warp_grid_f64(pose, h, w, x_reso, y_reso, x_min, y_min):
    """float64 statement of get_transformed_grid on the inverse of `pose` -> normalised (gx, gy), each [h, w]."""
    inv = np.linalg.inv(np.asarray(pose, np.float64))
    mx = np.tile(((np.arange(w, dtype=np.float64) + 0.5) * x_reso + x_min)[None, :], (h, 1))
    my = np.tile(((np.arange(h, dtype=np.float64) + 0.5) * y_reso + y_min)[:, None], (1, w))
    tx = inv[0, 0] * mx + inv[0, 1] * my + inv[0, 3]
    ty = inv[1, 0] * mx + inv[1, 1] * my + inv[1, 3]
    return tx / abs(x_min), ty / abs(y_min)


def warp_f64(bev, poses, x_reso, y_reso, x_min, y_min):
    """float64 statement of warp_feats: bev [B,T,C,H,W], poses [B,T,4,4] -> (warped [B,T,C,H,W] float64 with slot 0 = frame T-1 unwarped,
    pixel coordinates px, py [B,T,H,W] of every sample; slot 0 holds the cell's own position)."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(bev, np.float64))
    B, T, C, H, W = x.shape
    out = np.empty(x.shape, np.float64)
    px = np.tile(np.arange(W, dtype=np.float64)[None, None, None, :], (B, T, H, 1))
    py = np.tile(np.arange(H, dtype=np.float64)[None, None, :, None], (B, T, 1, W))
    for b in range(B):
        out[b, 0] = x[b, T - 1].numpy()
        for t in range(1, T):
            gx, gy = warp_grid_f64(poses[b, t], H, W, x_reso, y_reso, x_min, y_min)
            grid = torch.from_numpy(np.stack([gx, gy], -1)).view(1, H, W, 2)
            out[b, t] = torch.nn.functional.grid_sample(x[b, t:t + 1], grid, mode='bilinear', padding_mode='zeros', align_corners=False)[0].numpy()
            px[b, t], py[b, t] = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    return out, px, py


def aniso_poses():
    """The fixture's poses [2,3,4,4] f32: frames 1, 2 turned by +0.3 / -0.3 rad (sample 0) and +1.5 / -1.5 rad (sample 1), translations U(-3, 3)."""
    rng = np.random.RandomState(3)
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 3, 1, 1))
    for b, a0 in enumerate((0.3, 1.5)):
        for t, a in ((1, a0), (2, -a0)):
            poses[b, t, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            poses[b, t, :3, 3] = rng.uniform(-3, 3, 3)
    return poses


def aniso_bev():
    """The fixture's BEV map [2,3,4,96,64] f32 (too large to store: drawn again from its seed)."""
    return np.random.RandomState(5).randn(2, 3, 4, 96, 64).astype(np.float32)


def aniso_pillar_feats(m):
    """The fixture's 4-channel pillar features [m,4] f32 for the scatter."""
    return np.random.RandomState(3).randn(m, 4).astype(np.float32)


def aniso_ungrid_points(rng, k, x_half=8.0, y_half=6.0):
    """k points in [-1.2, 1.2] x (x_half, y_half) -- about a third outside the map on each axis -- then the four corners, the four edge
    midpoints and the centre of the map.  -> [k + 9, 3] f32."""
    p = rng.uniform(-1.2, 1.2, (k, 3)) * [x_half, y_half, 1.0]
    edge = [[sx * x_half, sy * y_half, 0] for sx in (-1, 1) for sy in (-1, 1)] + [[-x_half, 0, 0], [x_half, 0, 0], [0, -y_half, 0], [0, y_half, 0], [0, 0, 0]]
    return np.concatenate([p, np.array(edge, np.float64)]).astype(np.float32)


ANISO_SMALL_WARP = (16.0 / 12.0, 12.0 / 18.0, -8.0, -6.0)      # x_reso, y_reso, x_min, y_min of an 18 x 12 map over the same 16 m x 12 m


def aniso_gather_case(c):
    """Synthetic bilinear-gather inputs: 3 maps of 9 x 14 cells (ragged 4 x 4 tiles on both axes, different remainders) x c channels, scales 8 and 6,
    700 points drawn like the fixture's; map_idx[100:110] = -1 and map_idx[110:120] = 3 name no map.
    -> fmap [3,9,14,c] f32 (channels last), points [700,3] f32, map_idx [700] i32, grad [700,c] f32."""
    rng = np.random.RandomState(100 + c)
    fmap = rng.randn(3, 9, 14, c).astype(np.float32)
    pts = aniso_ungrid_points(rng, 691)
    idx = rng.randint(0, 3, pts.shape[0]).astype(np.int32)
    idx[100:110] = -1
    idx[110:120] = 3
    return fmap, pts, idx, rng.randn(pts.shape[0], c).astype(np.float32)


def aniso_warp_case(c):
    """Synthetic warp inputs: bev [2,3,c,18,12] f32 on ANISO_SMALL_WARP with the fixture's poses."""
    return np.random.RandomState(200 + c).randn(2, 3, c, 18, 12).astype(np.float32), aniso_poses()


def make_batch(cfg, seeds, n_frames, pts_per_frame, mode='uniform', voxeliser=None):
    vox = voxeliser or oracle_voxeliser(cfg)
    samples = [attach_voxels(make_sequence(s, n_frames, pts_per_frame, cfg, mode=mode), vox) for s in seeds]
    return collate_fn(samples)


def vox_points(seed, n, cfg, frac_out=0.1):
    """Same generator as tests/golden/make_golden.py:vox_points."""
    rng = np.random.RandomState(seed)
    r = np.asarray(cfg['voxel_generator']['range'], np.float64)
    T = cfg['voxel_generator']['n_sweeps']
    lo, hi = r[:3], r[3:]
    span = hi - lo
    p = lo + rng.uniform(-frac_out / 2, 1 + frac_out / 2, (n, 3)) * span
    t = rng.randint(0, T, n)
    edge = rng.randint(0, n, 32)
    p[edge[:8], 0] = lo[0]
    p[edge[8:16], 0] = hi[0]
    p[edge[16:24], 1] = lo[1] + 0.25 * rng.randint(0, int(span[1] / 0.25), 8)
    p[edge[24:], 2] = hi[2]
    return np.concatenate([p, t[:, None]], axis=1).astype(np.float32)


def raw_sample(seed, n_frames, ppf, cfg):
    """A raw sample as BaseDataset.__getitem__ reads it from disk (libs/dataset.py:206-214): float64 points with some beyond
    the crop box, below the ground threshold and above crop_z_max; per-point labels and frame index as 1-D arrays."""
    import numpy as np
    from pcaccumulation_amd.synthetic import make_sequence
    s = make_sequence(seed, n_frames, ppf, cfg)
    pts = s['input_points'].astype(np.float64)
    pts[::7] *= 1.6
    pts[::5, 2] -= 1.0
    pts[3::11, 2] += 9.0
    return {'raw_points': pts, 'time_indice': s['time_indice'][:, 0].astype(np.float64), 'sd_labels': s['sd_labels'][:, 0],
            'fb_labels': s['fb_labels'][:, 0], 'inst_labels': s['inst_labels'][:, 0], 'ego_motion_gt': s['ego_motion_gt'].astype(np.float64),
            'inst_motion_gt': s['inst_motion_gt'].astype(np.float64)}


def flow_error_scenes(root, n_scenes=3, seed=0):
    """A results folder as SegTrainer.test leaves it (libs/tester.py:95-107): <root>/<scene>/flow_error.npz with the reference's
    keys and narrow dtypes; errors spread around the 0.05 / 0.1 / 0.3 thresholds; the last scene has no moving point and no
    static foreground, and stores its frame index run-length coded ('length', toolbox/evaluation.py:37-46)."""
    import os
    rng = np.random.RandomState(seed)
    for s in range(n_scenes):
        n = 4000 + 777 * s
        t = np.sort(rng.randint(1, 5, n)).astype(np.int8)
        fb = rng.rand(n) < 0.2
        sd = fb & (rng.rand(n) < 0.5)
        if s == n_scenes - 1:
            fb[:] = False
            sd[:] = False
        epe = np.abs(rng.randn(n) * 0.15).astype(np.float16)
        rel = np.abs(rng.randn(n) * 0.2).astype(np.float16)
        d = os.path.join(root, 'scene_%03d' % s)
        os.makedirs(d, exist_ok=True)
        if s == n_scenes - 1:
            vals, counts = np.unique(t, return_counts=True)
            np.savez_compressed(os.path.join(d, 'flow_error'), fb_label=fb, sd_label=sd, epe_per_point=epe, relative_error=rel,
                                time_indice=vals.astype(np.int8), length=counts.astype(np.int64))
        else:
            np.savez_compressed(os.path.join(d, 'flow_error'), fb_label=fb, sd_label=sd, epe_per_point=epe, relative_error=rel, time_indice=t)
