"""What the tools/bench_accumulate*.py tools share (the accumulated-cloud family, include/pcacc.h C4 and later): the import
paths, the constants of the scene, the key decoding of the host baselines, the shared command-line flags, the 40-window drifting scene, the two
device-event timers and the report that is rewritten after every line.  A new bench_accumulate_*.py starts from these and keeps what is its own: its
docstring, its own flags, its measurement sequence and its host baseline.
torch and pcaccumulation_amd are imported where they are needed: a tool's parser is reachable, and --help runs, without them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')):      # the package, the tools, the restatements of the host baselines
    if _p not in sys.path:
        sys.path.insert(0, _p)

SENSOR = np.array([[0.0, 0.0, 1.8]])                                             # synthetic.make_sequence: the beams start here
BIAS = 1 << 20
HBM_GBS = 8000.0                                                                 # MI355X: 8 TB/s peak


def drift(k):
    """The pose of window k: 2 m and 0.5 degrees further per window."""
    a = np.deg2rad(0.5 * k)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    T[:3, 3] = (2.0 * k, 0.1 * k, 0.0)
    return T


def voxel_coords(keys):
    """The signed voxel indices [x, y, z] of int64 keys (21 bits each, biased by BIAS)."""
    return [((keys >> 42) & 0x1fffff) - BIAS, ((keys >> 21) & 0x1fffff) - BIAS, (keys & 0x1fffff) - BIAS]


def parser(out, capacity=False, repeat=None, repeats=None, baseline=True):
    """The flags of the scene and those that several tools share; a tool names the ones it has and adds its own.  `out`: the file name under
    profiles/ that --out defaults to; `repeat` / `repeats`: the default of --repeat / --repeats (a tool has the spelling its recorded command
    lines use)."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=40)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--pts-per-frame', type=int, default=160000)
    ap.add_argument('--voxel', type=float, default=0.1)
    if capacity:
        ap.add_argument('--capacity', type=int, default=1 << 20)
    if repeat is not None:
        ap.add_argument('--repeat', type=int, default=repeat)
    if repeats is not None:
        ap.add_argument('--repeats', type=int, default=repeats)
    if baseline:
        ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', out))
    return ap


def header(tool, a, flags, how):
    """A report's first line: the command line that repeats the run, the device and how the times were taken."""
    import torch
    return 'tools/%s --windows %d --frames %d --pts-per-frame %d --voxel %g %s   (%s; %s)' % (
        os.path.basename(tool), a.windows, a.frames, a.pts_per_frame, a.voxel, flags, torch.cuda.get_device_name(0), how)


def window_points(a, k, device):
    """The points of window k of the scene, [frames * pts_per_frame, 3] f32 on `device`, in the window's own frame."""
    import torch
    from pcaccumulation_amd.config import default_config
    from pcaccumulation_amd.synthetic import make_sequence
    s = make_sequence(500 + k, a.frames, a.pts_per_frame, default_config('waymo', 'test', n_sweeps=a.frames), mode='lidar_scan')
    return torch.from_numpy(np.ascontiguousarray(s['input_points'][:, :3], np.float32)).to(device)


def scene(a, device):
    """The drifting scene, window by window: yields (k, points [n,3] f32, moving [n] bool, pose [4,4] f64) for k < a.windows, the tensors on
    `device`.  10 % of the points are flagged as moving, drawn from one stream in window order: a tool that splits the scene takes its windows
    from ONE generator."""
    import torch
    rng = np.random.RandomState(0)
    for k in range(a.windows):
        pts = window_points(a, k, device)
        yield k, pts, torch.from_numpy(rng.rand(pts.shape[0]) < 0.1).to(device), drift(k)


def timed(fn):
    """One call between device events -> (ms, what it returned).  No warm-up: the caller discards a first call where it wants one."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def timed_repeat(fn, repeat):
    """One warm-up call, then `repeat` calls between device events -> (what the last one returned, [ms])."""
    import torch
    fn()                                                                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        t, res = timed(fn)
        ms.append(t)
    return res, ms


def stats(t):
    return 'median %.2f ms, min %.2f, max %.2f' % (float(np.median(t)), min(t), max(t))


class Report(object):
    """The lines of a run, the header first; emit() prints a line and rewrites the file."""

    def __init__(self, out, header):
        self.out, self.lines = out, [header]

    def emit(self, line):
        self.lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(self.out)), exist_ok=True)
        with open(self.out, 'w') as f:                                           # rewritten line by line: a run that is cut short leaves what it measured
            f.write('\n'.join(self.lines) + '\n')
