"""The tools/bench_accumulate*.py tools and what they share (tools/accum_bench.py): the scene, bit for bit, against a literal restatement of its
loop; every tool's flags and defaults against a table; the report that is complete after every line; the key decoding; and, on the GPU, every
tool run once in-process at a size of a few thousand points, its host baseline on, with no line that reports a mismatch."""
import argparse
import importlib
import os
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import accum_bench  # noqa: E402

SCENE = dict(windows=40, frames=5, pts_per_frame=160000, voxel=0.1)
MILLION = 1000000
# tool -> (its own flags and the shared ones it has, with their defaults; the file under profiles/ that --out defaults to)
DEFAULTS = {
    'bench_accumulate': (dict(capacity=1 << 20, no_baseline=False), 'accum_bench.txt'),
    'bench_accumulate_columns': (dict(repeat=5, no_baseline=False), 'accum_columns_bench.txt'),
    'bench_accumulate_compare': (dict(capacity=1 << 20, repeats=5, no_baseline=False), 'accum_compare_bench.txt'),
    'bench_accumulate_components': (dict(repeat=5, min_voxels=10, host_rows=MILLION, no_baseline=False), 'accum_components_bench.txt'),
    'bench_accumulate_field': (dict(repeat=5, box=(512, 512, 64), points=800000, no_baseline=False), 'accum_field_bench.txt'),
    'bench_accumulate_knn': (dict(box=50.0, repeat=5, no_baseline=False), 'accum_knn_bench.txt'),
    'bench_accumulate_merge': (dict(capacity=1 << 20, repeats=5, no_baseline=False), 'accum_merge_bench.txt'),
    'bench_accumulate_normals': (dict(baseline_rows=MILLION, no_baseline=False), 'accum_normals_bench.txt'),
    'bench_accumulate_observe': (dict(coarse=0.4, max_steps=4096, repeats=10), 'accum_observe_bench.txt'),
    'bench_accumulate_observe_merge': (dict(max_steps=4096, repeats=5), 'accum_observe_merge_bench.txt'),
    'bench_accumulate_pierce': (dict(max_range=30.0, max_steps=4096, sample=2000, no_baseline=False), 'accum_pierce_bench.txt'),
    'bench_accumulate_planes': (dict(repeat=5, host_rows=MILLION, no_baseline=False), 'accum_planes_bench.txt'),
    'bench_accumulate_prune': (dict(box=50.0, repeat=5, neighbour_rows=MILLION, no_baseline=False), 'accum_prune_bench.txt'),
    'bench_accumulate_query': (dict(box=50.0, repeat=5, no_baseline=False), 'accum_query_bench.txt'),
    'bench_accumulate_raycast': (dict(max_range=30.0, min_range=2.0, box=50.0, sample=2000, repeat=5, no_baseline=False), 'accum_raycast_bench.txt'),
    'bench_accumulate_register': (dict(max_iter=30, no_baseline=False), 'accum_register_bench.txt'),
}
# the smallest arguments of the GPU cases, after --windows 4 --pts-per-frame 2000: one repeat, the host legs on a few thousand rows
SMALL = {
    'bench_accumulate': [],
    'bench_accumulate_columns': ['--repeat', '1'],
    'bench_accumulate_compare': ['--repeats', '1'],
    'bench_accumulate_components': ['--repeat', '1', '--host-rows', '2000'],
    'bench_accumulate_field': ['--repeat', '1', '--box', '32', '32', '16', '--points', '2000'],
    'bench_accumulate_knn': ['--repeat', '1'],
    'bench_accumulate_merge': ['--repeats', '1'],
    'bench_accumulate_normals': ['--baseline-rows', '2000'],
    'bench_accumulate_observe': ['--repeats', '1'],
    'bench_accumulate_observe_merge': ['--repeats', '1'],
    'bench_accumulate_pierce': ['--sample', '50'],
    'bench_accumulate_planes': ['--repeat', '1', '--host-rows', '2000'],
    'bench_accumulate_prune': ['--repeat', '1', '--neighbour-rows', '2000'],
    'bench_accumulate_query': ['--repeat', '1'],
    'bench_accumulate_raycast': ['--repeat', '1', '--sample', '50'],
    'bench_accumulate_register': [],
}
MISMATCH = re.compile(r'DIFFERENT|NOT equal|identical: False')


def test_every_tool_is_in_the_tables():
    tools = sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, 'tools')) if f.startswith('bench_accumulate') and f.endswith('.py'))
    assert tools == sorted(DEFAULTS) == sorted(SMALL)


def test_scene_against_its_restatement():
    from pcaccumulation_amd.config import default_config
    from pcaccumulation_amd.synthetic import make_sequence
    a = argparse.Namespace(windows=3, frames=2, pts_per_frame=200)
    got = list(accum_bench.scene(a, 'cpu'))
    cfg = default_config('waymo', 'test', n_sweeps=2)
    rng = np.random.RandomState(0)
    assert [g[0] for g in got] == [0, 1, 2]
    for k, pts, moving, pose in got:
        s = make_sequence(500 + k, 2, 200, cfg, mode='lidar_scan')
        want = np.ascontiguousarray(s['input_points'][:, :3], np.float32)
        assert pts.numpy().dtype == np.float32 and pts.is_contiguous() and np.array_equal(pts.numpy(), want)
        assert moving.numpy().dtype == np.bool_ and np.array_equal(moving.numpy(), rng.rand(want.shape[0]) < 0.1)
        assert np.array_equal(pose, accum_bench.drift(k))
    fresh = make_sequence(503, 2, 200, cfg, mode='lidar_scan')                   # the window after the last: query's and knn's fresh scan
    assert np.array_equal(accum_bench.window_points(a, 3, 'cpu').numpy(), np.ascontiguousarray(fresh['input_points'][:, :3], np.float32))


@pytest.mark.parametrize('k', [0, 1, 39])
def test_drift(k):
    angle = 0.5 * k * np.pi / 180.0
    want = np.array([[np.cos(angle), -np.sin(angle), 0.0, 2.0 * k], [np.sin(angle), np.cos(angle), 0.0, 0.1 * k], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    got = accum_bench.drift(k)
    assert got.dtype == np.float64 and got.shape == (4, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)                    # deg2rad against pi / 180: an ulp of the angle


@pytest.mark.parametrize('tool', sorted(DEFAULTS))
def test_parser_defaults(tool):
    own, out = DEFAULTS[tool]
    want = dict(SCENE, out=os.path.join(ROOT, 'profiles', out), **own)
    got = vars(importlib.import_module(tool).parse_args([]))
    assert {k: (type(v), v) for k, v in got.items()} == {k: (type(v), v) for k, v in want.items()}


def test_report_is_complete_after_every_line(tmp_path):
    path = str(tmp_path / 'not_there_yet' / 'report.txt')
    report = accum_bench.Report(path, 'the header')
    report.emit('one')
    assert open(path).read() == 'the header\none\n'
    report.emit('two')
    assert open(path).read() == 'the header\none\ntwo\n'


def test_voxel_coords_inverts_the_packing():
    edge = accum_bench.BIAS
    assert edge == 1 << 20
    corners = [(x, y, z) for x in (-edge, 0, edge - 1) for y in (-edge, 0, edge - 1) for z in (-edge, 0, edge - 1)]
    c = np.array(corners, np.int64)
    keys = ((c[:, 0] + edge) << 42) | ((c[:, 1] + edge) << 21) | (c[:, 2] + edge)
    assert keys.dtype == np.int64 and keys.min() == 0 and keys.max() == (1 << 63) - 1
    got = accum_bench.voxel_coords(keys)
    assert len(got) == 3 and all(g.dtype == np.int64 for g in got)
    assert np.array_equal(np.stack(got, 1), c)


@pytest.mark.gpu
@pytest.mark.parametrize('tool', sorted(SMALL))
def test_tool_runs_small(tool, tmp_path):
    out = str(tmp_path / (tool + '.txt'))
    t0 = time.perf_counter()
    importlib.import_module(tool).main(['--windows', '4', '--pts-per-frame', '2000'] + SMALL[tool] + ['--out', out])
    print('%s: %.1f s' % (tool, time.perf_counter() - t0))
    lines = open(out).read().splitlines()
    assert lines[0].startswith('tools/%s.py --windows 4 --frames 5 --pts-per-frame 2000 ' % tool), lines[0]
    assert len(lines) > 1
    bad = [line for line in lines if MISMATCH.search(line)]
    assert not bad, bad
