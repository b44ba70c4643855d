"""Time the columns, the local ground and the bird's-eye-view rasters of the accumulated scene cloud (include/pcacc.h C17, AccumulatedCloud.columns / bev) on
the 40-window drifting scene of tools/bench_accumulate.py (5 x 160 k points per window, 0.1 m) and, beside it on the same machine and inputs, what a user
does without it: the copy of the records to the host, np.unique over the column keys and a minimum filter there.
  GPU leg    columns() at ground_radius 0, 2 and 8 (the read-back of the two counts included), and bev() of the bounding box of the columns (its columns()
             call and both read-backs included; the raster alone through the binding beside it); device events around each call, one warm-up, median of
             --repeat with min and max.
  host leg   records() (the copy), np.unique over key >> 21 with the first row and the run length of every column, z_low from the first row, and the
             (2R + 1)^2 minimum filter of R = 2 on a dense grid of the bounding box (scipy.ndimage.minimum_filter when scipy is installed, else the 25
             shifted np.minimum passes); ground_z must equal the GPU's.
The windows of this scene are independent random clouds: the scene gives the sizes and the memory behaviour of a real sequence.  Results go to --out.
Nothing is gated on them.
Usage: python tools/bench_accumulate_columns.py [--windows 40] [--repeat 5] [--no-baseline] [--out profiles/accum_columns_bench.txt]"""
import time

import numpy as np

from accum_bench import Report, header, parser, scene, timed_repeat


def parse_args(argv=None):
    return parser('accum_columns_bench.txt', repeat=5).parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    dev = torch.device('cuda:0')
    emit = Report(a.out, header(__file__, a, '--repeat %d' % a.repeat,
                                'GPU: device events around each call, one warm-up, median of %d; host: perf_counter, once' % a.repeat)).emit
    m = AccumulatedCloud(a.voxel, dev, 1 << 20)
    for k, pts, mv, T in scene(a, dev):
        m.add(pts, T, mv, k)
        if k % 10 == 9:
            print('window %d: %d voxels' % (k, m.num_voxels), flush=True)
    names = ('rows', 'columns', 'ground rows', 'rows in the band', 'columns with a borrowed ground')

    def report(what, fn, counters=lambda res: res['counters']):
        res, ms = timed_repeat(fn, a.repeat)
        counts = ', '.join('%s %d' % (k, v) for k, v in zip(names, counters(res).tolist()))
        emit('  GPU %s: median %.3f ms, min %.3f, max %.3f; %s' % (what, float(np.median(ms)), min(ms), max(ms), counts))
        return res, float(np.median(ms))

    emit('the full map: %d voxels, no filter, thickness 1, band (2, 20)' % m.num_voxels)
    got = {}
    for R in (0, 2, 8):
        got[R], _ = report('columns(ground_radius=%d), the read-back of the two counts included' % R, lambda: m.columns(ground_radius=R))
    cols = got[2]
    C = cols['xy'].shape[0]
    emit('  %d columns, %.2f voxels per column on average, the tallest %d' % (C, m.num_voxels / max(C, 1), int(cols['voxels'].max())))
    image, _ = report('bev(ground_radius=2) of the bounding box, its columns() call and both read-backs included', lambda: m.bev(ground_radius=2),
                      lambda res: res['columns']['counters'])
    H, W = image['column'].shape
    x0, y0 = image['origin']
    emit('  the bounding box: origin (%d, %d), %d x %d = %d pixels, %d of them columns' % (x0, y0, H, W, H * W, int((image['column'] >= 0).sum())))
    out = {name: torch.empty((H, W), dtype=dtype, device=dev) for name, dtype, _ in native.BEV_FIELDS}
    _, ms = timed_repeat(lambda: native.accum_bev(m._cur, m.num_voxels, 1, None, cols, x0, y0, W, H, out=out), a.repeat)
    emit('  GPU the raster alone (native.accum_bev into given images: pass 1 of C5 and the pixel kernel): median %.3f ms, min %.3f, max %.3f'
         % (float(np.median(ms)), min(ms), max(ms)))
    if not a.no_baseline:
        t0 = time.perf_counter()
        keys, acc, stamps = m.records()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        ck, first, voxels = np.unique(keys >> 21, return_index=True, return_counts=True)
        z_low = (keys[first] & 0x1fffff) - (1 << 20)
        x, y = (ck >> 21) - (1 << 20), (ck & 0x1fffff) - (1 << 20)
        t_unique = time.perf_counter() - t0
        t0 = time.perf_counter()
        big = 1 << 40                                                            # above every voxel index; scipy passes cval through a double
        grid = np.full((int(x.max() - x.min()) + 1, int(y.max() - y.min()) + 1), big, np.int64)
        grid[x - x.min(), y - y.min()] = z_low
        try:
            from scipy.ndimage import minimum_filter
            low, how = minimum_filter(grid, size=5, mode='constant', cval=big), 'scipy.ndimage.minimum_filter'
        except ImportError:
            pad = np.pad(grid, 2, constant_values=big)
            low, how = grid.copy(), '25 shifted np.minimum passes'
            for dx in range(5):
                for dy in range(5):
                    np.minimum(low, pad[dx:dx + grid.shape[0], dy:dy + grid.shape[1]], out=low)
        ground = low[x - x.min(), y - y.min()]
        t_filter = time.perf_counter() - t0
        same = np.array_equal(ground, cols['ground_z'].cpu().numpy()) and np.array_equal(first, cols['first_row'].cpu().numpy()) and \
            np.array_equal(voxels, cols['voxels'].cpu().numpy())
        emit('host, the same map, R = 2: copy of the records %.2f s; np.unique over the column keys, z_low, xy %.2f s; the 5 x 5 minimum filter on the dense '
             '%d x %d grid (%s) %.2f s; %d columns; first_row, voxels and ground_z are %s to the GPU\'s' % (t_copy, t_unique, grid.shape[0], grid.shape[1], how,
                                                                                                          t_filter, ck.shape[0], 'equal' if same else 'NOT equal'))
        assert same
    emit('not measured here: the split between pass 1, the scan and the kernels (a rocprofv3 --kernel-trace --stats run of this tool gives it: appended to '
         'profiles/accum_columns_bench.txt), the achieved bandwidth, any counter run, other scenes, a filter; prefix-sum differences for the sums and a '
         'segmented wave reduction were not built, so there is no A/B for them')


if __name__ == '__main__':
    main()
