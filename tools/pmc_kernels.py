#!/usr/bin/env python
"""Workload for the PMC passes over the MFMA kernels (rocprofv3 --pmc <set> --kernel-trace, one counter set per run):
  conv3x3_resident_kernel   64 -> 64 @ 288^2, 20 images      (csrc/conv.hip, weights resident in LDS)
  conv3x3_strip_kernel      256 -> 256 @ 36^2, 20 images     (csrc/conv_deep.hip, forward / data gradient of the deep layers)
  conv3x3_wgrad_kernel      32 -> 32 @ 288^2, 20 images      (csrc/conv.hip)
  conv3x3_wgrad_strip_kernel 256 x 256 @ 36^2, 20 images     (csrc/conv_deep.hip)
  rows_wgrad_bf16_kernel    3.2 M rows, 32 -> 32             (csrc/mlp_mfma.hip, the pillar encoder's weight gradients)
  rows_linear_bf16_kernel   3.2 M rows, 64 -> 32
three launches each.  tools/pmc_kernels_summary.py turns the counter files into profiles/rNN_pmc_kernels_summary.json."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcaccumulation_amd import native  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)


def conv(n, h, ci, co):
    x = bf(n, h, h, ci)
    w = torch.randn(co, ci, 3, 3, device=dev) / (3 * ci ** 0.5)
    b = torch.randn(co, device=dev)
    wp = native.conv3x3_prepare_weights(w)
    for _ in range(3):
        native.conv3x3(x, wp, b, 1, True)


def wgrad(n, h, ci, co, deep):
    x, gy = bf(n, h, h, ci), bf(n, h, h, co)
    for _ in range(3):
        (native.conv3x3_wgrad_deep if deep else native.conv3x3_wgrad)(gy, x)


conv(20, 288, 64, 64)
conv(20, 36, 256, 256)
wgrad(20, 288, 32, 32, False)
wgrad(20, 36, 256, 256, True)
rows = 3_200_000
x, dy = bf(rows, 32), bf(rows, 32)
for _ in range(3):
    native.rows_wgrad(dy, x)
x64 = bf(rows, 64)
w = torch.randn(32, 64, device=dev) / 8
for _ in range(3):
    native.rows_linear(x64, w, None, None, False, True, out_dtype=torch.bfloat16)
# ---- fp32x3 kernels (round 3): fp32 operands, scaled fp16 hi / lo products
f32 = lambda *shape: torch.randn(*shape, device=dev)


def conv_split(n, h, ci, co, kt=1, frames=1):
    x, gy = f32(n, h, h, ci), f32(n, h, h, co)
    w = torch.randn(*((co, ci, 3, 3, 3) if kt == 3 else (co, ci, 3, 3)), device=dev) / (3 * (ci * kt) ** 0.5)
    b = torch.randn(co, device=dev)
    wf, wb = native.conv3x3_split_prepare_weights(w)
    ax, ag = native.absmax256(x), native.absmax256(gy)
    for _ in range(3):
        native.conv3x3_split(x, wf, b, frames, True, amax=ax)
    for _ in range(3):
        native.conv3x3_wgrad_split(gy, x, frames, 0, dy_amax=ag, x_amax=ax)


conv_split(20, 288, 32, 32)               # conv3x3_split_res_kernel<32,1,2,5> + conv3x3_wgrad_split_kernel<1,1,9>
conv_split(20, 36, 256, 256)              # conv3x3_split_kernel<64,2,2,2,9> + conv3x3_wgrad_split_kernel<2,2,9>
xr, dyr = f32(rows, 32), f32(rows, 32)
ar, ad = native.absmax256(xr), native.absmax256(dyr)
w32 = torch.randn(32, 32, device=dev) / 6
for _ in range(3):
    native.rows_linear_split(xr, ar, w32, None, None, False, True)
for _ in range(3):
    native.rows_wgrad_split(dyr, ad, xr, ar)
for _ in range(3):
    native.absmax256(xr)
# fused pillar-encoder block (two-piece rows), wide row layer with weights in registers, fg/bg head kernels
m = 1_169_433
xa, pooled = f32(rows, 32), f32(m, 32)
p2v = torch.randint(0, m, (rows,), device=dev, dtype=torch.int32)
w0, ws, w1 = torch.randn(32, 64, device=dev) / 8, torch.randn(32, 64, device=dev) / 8, torch.randn(32, 32, device=dev) / 6
b0, b1 = torch.randn(32, device=dev), torch.randn(32, device=dev)
aa, ap = native.absmax256(xa), native.absmax256(pooled)
for _ in range(3):
    out, hr, xm, hm, oa, ha = native.pfn_block_split_forward(xa, aa, pooled, ap, p2v, w0, b0, ws, w1, b1)
g = f32(rows, 32)
ag = native.absmax256(g)
for _ in range(3):
    native.pfn_block_split_dgrad(g, ag, xm, hm, w0, ws, w1, True)
x128 = f32(429_567, 128)
a128 = native.absmax256(x128)
w128 = torch.randn(128, 128, device=dev) / 11
for _ in range(3):
    native.rows_linear_split(x128, a128, w128, None, None, False, True)      # rows_linear_split_fm_kernel<128, 4>
xh = bf(20, 288, 288, 32)
wh = torch.randn(2, 32, 3, 3, device=dev) / 17
dyh = f32(20, 288, 288, 2)
for _ in range(3):
    native.head_conv3x3_forward(xh, wh, torch.zeros(2, device=dev))
    native.head_conv3x3_dgrad(dyh, wh, 32, torch.bfloat16)
    native.head_conv3x3_wgrad(dyh, xh)
# ---- round 4: the 'mixed' mode's kernels -- fp32x3 forward with a bf16 second output, pool backward with fp32 winners, batched collate + voxelise
# (the bf16 second outputs of the split kernels share their kernels' names with the plain launches above: one extra 2-byte store per element;
#  they are timed in tools/native_call_table.py, not here)
yp = torch.relu(f32(20, 288, 288, 32))
gp, gs = bf(20, 144, 144, 32), bf(20, 288, 288, 64)[..., 32:]
for _ in range(3):
    native.pool_skip_relu_backward(yp, gp, gs)                                                                          # pool_skip_relu_bwd_y32_kernel
from pcaccumulation_amd.config import default_config  # noqa: E402
from pcaccumulation_amd.pipeline import sample_to_device  # noqa: E402
from pcaccumulation_amd.synthetic import make_sequence  # noqa: E402
cfgv = default_config('waymo', 'train', n_sweeps=5)
smp = [sample_to_device(make_sequence(i, 5, 160000, cfgv), dev) for i in range(4)]
vg = cfgv['voxel_generator']
import numpy as np  # noqa: E402
grid = np.round((np.array(vg['range'][3:], np.float32) - np.array(vg['range'][:3], np.float32)) / np.array(vg['voxel_size'], np.float32)).astype(int).tolist()
for _ in range(3):
    native.collate_voxelize(smp, vg['voxel_size'], vg['range'], grid, 5)                                               # vox_batch_keys / vox_batch_assign / vox_p2v
# ---- round 4, second half: the kernels the round-3 verdict named (item 7) and the kernels added late in round 4
k_pts = 320_000
pts = torch.rand(k_pts, 3, device=dev) * 2 - 1                                     # normalised positions, uniform over the map
midx = torch.randint(0, 4, (k_pts,), device=dev, dtype=torch.int32).sort().values
gk = f32(k_pts, 64)
for _ in range(3):
    native.bilinear_gather_backward_sorted(gk, (4, 288, 288, 64), pts, midx, 1.0, 1.0, out_dtype=torch.bfloat16)   # bilinear_sorted_prep + bilinear_gather_bwd_sorted
la = f32(16, 1024, 1024)
for _ in range(3):
    lp, lr, lc = native.sinkhorn_forward(la, 3)                                    # ego_sinkhorn_rows_ro / cols_ro / finish_ro
    native.sinkhorn_backward(torch.randn_like(lp), la, lr, lc)                     # sk_rowsum / sk_cols / sk_rows / sk_final
n_seg = 600_000
lg, lbl = f32(n_seg, 2), torch.randint(0, 2, (n_seg,), device=dev)
for _ in range(3):
    native.seg_loss_forward(lg, 0, lbl, None, n_seg)                               # seg_rows / seg_tile_fg / seg_lovasz / seg_final
xu, dyu = bf(20, 144, 144, 64), bf(20, 288, 288, 64)[..., :32]                      # the 64 -> 32 decoder stage at full resolution; dy = a channel slice
wu = torch.randn(64, 32, 2, 2, device=dev) / 8
uf, ub = native.upconv2x2_bf16_prepare_weights(wu)
for _ in range(3):
    native.upconv2x2_bf16(xu, uf, torch.zeros(32, device=dev), 0)                  # upconv_bf16_kernel<4, 0>
    native.upconv2x2_bf16(dyu, ub, None, 1)                                        # upconv_bf16_kernel<2, 1>
    native.upconv2x2_bf16_wgrad(dyu, xu)                                           # upconv_bf16_wgrad_kernel + _reduce_kernel
x9 = f32(rows, 9)
w9, b9 = torch.randn(64, 9, device=dev) / 3, torch.randn(64, device=dev)
for _ in range(3):
    native.rows_linear_few_dual(x9, w9, b9)                                        # rows_linear_fewk_kernel<9, 8> with the bf16 shadow and the maxima
ca_, cb_ = f32(20, 288, 288, 32), f32(20, 288, 288, 32)
wc = torch.randn(32, 64, 3, 3, device=dev) / 24
wcf = native.conv3x3_split_prepare_weights(wc)[0]
amx = torch.maximum(native.absmax256(ca_), native.absmax256(cb_))
for _ in range(3):
    native.conv3x3_split_cat(ca_, cb_, amx, wcf, torch.zeros(32, device=dev), True, want_bf16=True)   # conv3x3_split_res_kernel<32,1,2,5,true> on two inputs
# ---- round 6: the pooling that writes the canvas, the pooling it is built from, the fixed-point few-row sums, the stable few-segment CSR
n_cells6 = 20 * 288 * 288
p2v6 = torch.cat([torch.arange(m, device=dev), torch.randint(0, m, (rows - m,), device=dev)])[torch.randperm(rows, device=dev)].to(torch.int32)
c2p6 = torch.full((n_cells6,), -1, dtype=torch.int32, device=dev)
c2p6[torch.randperm(n_cells6, device=dev)[:m].sort().values] = torch.arange(m, dtype=torch.int32, device=dev)
offs6, order6 = native.csr_build(p2v6, m)
rows6 = f32(rows, 32)
for _ in range(3):
    native.segment_max_canvas(rows6, offs6, order6, m, c2p6)                        # seg_max_canvas_kernel<8>
    native.segment_max_dual(rows6, offs6, order6, m)                                # seg_max_kernel<8>
slot6 = torch.randint(0, 400, (320_000,), device=dev, dtype=torch.int32)
v16 = f32(320_000, 16)
for _ in range(3):
    native.scatter_sum_small(v16, slot6, 400)                                       # scatter_sum_small_kernel + its fixed-order reduce
    native.csr_build(slot6, 400)                                                    # csr_histogram_small / csr_table_scan / csr_fill_small
torch.cuda.synchronize()
print('done')
