"""Rays through the accumulated scene cloud (include/pcacc.h C7): AccumulatedCloud.see_through / see_through_results / pierced.

CPU leg: csrc/accum_pierce.h -- the code the kernel runs -- built with g++ (-ffp-contract=off, every table index assert-checked, poison behind row m)
against the plain-Python restatement tests/accumulate_pierce_reference.py (a dict of coordinates, Python floats, no keys): the count of every voxel
and the five counters EQUAL, on random rays, exact ties, degenerate rays, the index bound with decoys, the stamp rule at equality and ray counts
around the wave size; the geometry of the walk checked on the restatement alone.
GPU leg: the kernel against the host build, integer for integer, on every scene; order and split independence; the sidecar carried through add and
growth, save / load, pierced() against extract(), the PLY column, a ghost trail that only the rays reveal, and the model tie-in."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_pierce_reference as pref
import accumulate_reference as ref
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

NAN, INF = float('nan'), float('inf')


# ---- maps ------------------------------------------------------------------------------------------------------------------------------
def _map_adds(name):
    """-> (voxel_size, [(points, stamp)]): the adds that build a map."""
    if name == 'third':                                                          # a random third of the 40^3 block around the origin
        keep = np.random.RandomState(5).uniform(0, 1, 64000) < 1.0 / 3.0
        return 0.1, [(ah.centres(ah.block(-20, 20)[keep], 0.1), 0)]
    if name == 'block9':
        return 0.25, [(ah.centres(ah.block(-4, 5), 0.25), 0)]
    if name == 'slab':                                                           # x -3..12, y and z -2..2
        idx = np.array([(x, y, z) for x in range(-3, 13) for y in range(-2, 3) for z in range(-2, 3)])
        return 0.1, [(ah.centres(idx, 0.1), 0)]
    if name == 'bound':
        walked, decoys = ah.walked_voxels()
        return 0.01, [(ah.centres(walked + decoys, 0.01), 0)]
    if name == 'empty':
        return 0.1, []
    assert name == 'stamped'                                                     # voxel (k, 0, 0) was filled from stamp 3 to stamp 3 + k
    adds = []
    for k in range(4):
        adds.append((ah.centres([(j, 0, 0) for j in range(k, 4)], 0.1), 3 + k))
    return 0.1, adds


_maps = {}


def _ref_map(name):
    """The restatement's map, built once and shared (never modified) -> (ReferenceMap, {coord: (t_first, t_last)})."""
    if name not in _maps:
        vs, adds = _map_adds(name)
        r = ref.ReferenceMap(vs)
        for pts, stamp in adds:
            r.add(pts, None, None, stamp)
        _maps[name] = (r, pref.voxels_of(r))
    return _maps[name]


# ---- cases: a map and the arguments of ONE see_through call ----------------------------------------------------------------------------------
def _rot_z(angle, t):
    T = np.eye(4)
    T[0, 0] = T[1, 1] = np.cos(angle)
    T[0, 1], T[1, 0] = -np.sin(angle), np.sin(angle)
    T[:3, 3] = t
    return T


def _cases():
    c = {}
    pts, origins, index = ah.random_rays()
    c['random'] = dict(map='third', points=pts, origins=origins, origin_index=index, margin=0.2)
    # exact ties: every t_a equal at every step; a face start with a negative direction (t = -0.0 steps at once)
    c['ties'] = dict(map='block9', points=np.array([[1, 1, 1]], np.float32), origins=np.zeros((1, 3)), margin=0.0)
    f = float(np.float32(0.3))
    c['face'] = dict(map='block9', points=np.array([[-0.6, 0.3, 0.3]], np.float32), origins=np.array([[0.5, f, f]]), margin=0.0)
    # degenerate rays
    o = np.array([[0.05, 0.05, 0.05]], np.float32).astype(np.float64)
    long_ray = np.array([[1.15, 0.05, 0.05]], np.float32)
    c['zero_length'] = dict(map='slab', points=o.astype(np.float32), origins=o)
    c['margin_ge_L'] = dict(map='slab', points=np.array([[0.2, 0.05, 0.05], [0.5, 0.0, 0.0]], np.float32), origins=np.array([[0.05, 0.05, 0.05], [0.0, 0, 0]]),
                            origin_index=np.array([0, 1], np.int32), margin=0.5)     # L = 0.15 < margin, and L == margin exactly (t_end = 0)
    c['range_cut'] = dict(map='slab', points=long_ray, origins=o, margin=0.2, max_range=0.32)
    c['range_zero'] = dict(map='slab', points=long_ray, origins=o, margin=0.2, max_range=0.0)
    c['steps1'] = dict(map='slab', points=long_ray, origins=o, margin=0.0, max_steps=1)
    c['steps5'] = dict(map='slab', points=long_ray, origins=o, margin=0.0, max_steps=5)
    c['steps_exact'] = dict(map='slab', points=long_ray, origins=o, margin=0.0, max_steps=12)      # ends by itself at its 12th visit: not truncated
    good = np.array([[0.95, 0.15, -0.05], [0.85, -0.15, 0.12], [1.05, 0.02, 0.17], [0.45, 0.1, 0.1]], np.float32)
    bad = np.array([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [32768, 0, 0], [0, -32768, 0]], np.float32)
    c['bad_first'] = dict(map='slab', points=np.concatenate([bad, good]), origins=o)
    c['bad_last'] = dict(map='slab', points=np.concatenate([good, bad]), origins=o)
    for j in range(5):
        c['bad_alone%d' % j] = dict(map='slab', points=bad[j:j + 1], origins=o)
    bad_o = np.array([[NAN, 0, 0], [0.05, 0.05, 0.05], [0, INF, 0], [0, 0, 32768.0], [-32768.0, 0, 0]])
    c['bad_origins'] = dict(map='slab', points=np.concatenate([good, good[:1]]), origins=bad_o, origin_index=np.array([0, 1, 2, 3, 4], np.int32))
    c['bad_origin_alone'] = dict(map='slab', points=good[:1], origins=bad_o[:1])
    c['bad_index'] = dict(map='slab', points=good, origins=np.concatenate([o, o]), origin_index=np.array([-1, 0, 2, 1], np.int32))
    c['all_moving'] = dict(map='slab', points=good, origins=o, moving=np.ones(4, bool))
    c['some_moving'] = dict(map='slab', points=np.concatenate([good, bad[:1]]), origins=o, moving=np.array([1, 0, 0, 1, 1], bool))
    c['n0'] = dict(map='slab', points=np.zeros((0, 3), np.float32), origins=o)
    c['m0'] = dict(map='empty', points=good, origins=o)
    # the index bound at 0.01 m: every ray ends in the LAST voxel of an axis, margin 0, pointing outwards; two more end outside and are dropped
    walked, _ = ah.walked_voxels()
    ends, starts = [], []
    for axis in range(3):
        for lo, last in ((-EDGE, -EDGE), (EDGE - 3, EDGE - 1)):
            s, e = [1, -2], [1, -2]
            s.insert(axis, lo + (2 if last < 0 else 0))
            e.insert(axis, last)
            starts.append(s)
            ends.append(e)
    ends = ah.centres(ends, 0.01)
    outside = np.array([[10485.77, 0.015, -0.015], [0.015, 0.015, -10485.78]], np.float32)
    c['bound'] = dict(map='bound', points=np.concatenate([ends, outside]), origins=ah.centres(starts, 0.01).astype(np.float64),
                      origin_index=np.array([0, 1, 2, 3, 4, 5, 0, 5], np.int32), margin=0.0)
    # the stamp rule: one ray through voxels (0..3, 0, 0) whose (t_first, t_last) are (3, 3), (3, 4), (3, 5), (3, 6)
    through = dict(map='stamped', points=np.array([[0.55, 0.05, 0.05]], np.float32), origins=np.array([[-0.15, 0.05, 0.05]]), margin=0.0)
    for s in (None, 2, 3, 4, 5, 6, 7):
        c['stamp_%s' % s] = dict(through, stamp=s)
    # ray counts around the wave size, under a pose
    pose = _rot_z(0.3, (0.2, -0.1, 0.05))
    for n in (1, 63, 64, 65, 257):
        c['count%d' % n] = dict(map='third', points=pts[:n], origins=origins, origin_index=index[:n], pose=pose, margin=0.2, max_range=1.5)
    return c


CASES = _cases()
CASE_NAMES = sorted(CASES)
_ARGS = ('origin_index', 'pose', 'moving', 'stamp', 'margin', 'max_range', 'max_steps')


def _restate(case, walks=None):
    r, vox = _ref_map(case['map'])
    kw = {k: case[k] for k in _ARGS if k in case}
    return pref.pierce(vox, case['points'], case['origins'], voxel_size=r.voxel_size, walks=walks, **kw)


def _in_key_order(name, pierced):
    keys = _ref_map(name)[0].records()[0]
    coords = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - ref.BIAS
    return pref.aligned(pierced, coords)


# ---- the host build ----------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_pierce_host_driver', 'accp')
_host_cache = {}


def _host(exe, tmp_path, case, tag, spare=3):
    """The g++ build of accum_pierce.h on one call (every assert of the driver aborts it) -> (pierced [m] i32 in key order, counters [5] i64, visits)."""
    if tag in _host_cache:
        return _host_cache[tag]
    r = _ref_map(case['map'])[0]
    keys, _, stamps = r.records()
    m = keys.shape[0]
    pts = np.ascontiguousarray(case['points'], np.float32).reshape(-1, 3)
    n = pts.shape[0]
    org = np.ascontiguousarray(case['origins'], np.float64).reshape(-1, 3)
    mv, idx, pose, stamp = case.get('moving'), case.get('origin_index'), case.get('pose'), case.get('stamp')
    margin = case['margin'] if case.get('margin') is not None else 2.0 * r.voxel_size
    head = [n, org.shape[0], m, m + spare, stamp is not None, stamp or 0, case.get('max_steps', 4096), mv is not None, idx is not None, pose is not None]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64),
                        np.array([r.voxel_size, margin, -1.0 if case.get('max_range') is None else case['max_range']], np.float64),
                        pts, np.zeros(n, np.uint8) if mv is None else np.asarray(mv).astype(np.uint8), org,
                        np.zeros(n, np.int32) if idx is None else np.asarray(idx, np.int32), np.eye(4) if pose is None else np.ascontiguousarray(pose, np.float64),
                        ah.map_bytes(keys, stamps=stamps), suffix='.bin')
    assert len(raw) == 4 * m + 48
    res = (np.frombuffer(raw, np.int32, m), np.frombuffer(raw, np.int64, 5, 4 * m), int(np.frombuffer(raw, np.int64, 1, 4 * m + 40)[0]))
    _host_cache[tag] = res
    return res


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------
def test_maps_hold_the_intended_voxels():
    """float32 voxel centres land in their voxels, at 0.01 m next to +-2^20 too."""
    for name in ('third', 'block9', 'slab', 'bound', 'stamped'):
        vs, adds = _map_adds(name)
        want = set()
        for pts, _ in adds:
            want |= set(map(tuple, np.floor(pts.astype(np.float64) / vs).astype(np.int64).tolist()))
        assert set(_ref_map(name)[1]) == want and _ref_map(name)[0].dropped == 0
    walked, decoys = ah.walked_voxels()
    assert set(_ref_map('bound')[1]) == set(walked) | set(decoys) and len(decoys) == 4 and not set(walked) & set(decoys)
    assert 20000 < len(_ref_map('third')[1]) < 22500
    assert sorted(_ref_map('stamped')[1].items()) == [((k, 0, 0), (3, 3 + k)) for k in range(4)]


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    """Every voxel's count and the five counters, equal."""
    case = CASES[name]
    pierced, counters = _restate(case)
    got_p, got_c, _ = _host(host_exe, tmp_path, case, name)
    assert got_c.tolist() == counters, (name, got_c.tolist(), counters)
    assert np.array_equal(got_p, _in_key_order(case['map'], pierced)), name
    assert sum(counters[:3]) == np.asarray(case['points']).reshape(-1, 3).shape[0]
    assert sum(pierced.values()) == counters[pref.HITS]


def test_random_scene_has_the_special_rays():
    pts, origins, index = ah.random_rays()
    d = pts[:24].astype(np.float64) - origins[0]
    assert np.all(d[0:6, 0] == 0) and np.all(d[6:10, 1] == 0) and np.all(d[10:14, 2] == 0)
    assert np.all((d[14:22] == 0).sum(1) == 2)
    pierced, counters = _restate(CASES['random'])
    assert counters[pref.WALKED] > 380 and counters[pref.DROPPED] == 0 and counters[pref.TRUNCATED] == 0 and counters[pref.HITS] > 2000


def test_exact_ties_visit_the_literal_sequence():
    """Voxel size 0.25, (0,0,0) -> (1,1,1), margin 0: all three t_a are equal at every step and the tie goes to x, then y, then z.  The walk ends where
    t = 1 is no longer < t_end = 1, in front of the end point's voxel (4,4,4)."""
    walks = []
    pierced, counters = _restate(CASES['ties'], walks)
    assert walks[0][1] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    assert counters == [1, 0, 0, 0, 10] and set(pierced.values()) == {1}
    # the origin on the face x = 0.5 of voxel 2, direction -x: t_x = -0.0 at the first step, the ray leaves voxel 2 at once
    walks = []
    pierced, counters = _restate(CASES['face'], walks)
    assert walks[0][1] == [(2, 1, 1), (1, 1, 1), (0, 1, 1), (-1, 1, 1), (-2, 1, 1), (-3, 1, 1)]
    assert counters == [1, 0, 0, 0, 6]


def test_degenerate_rays_in_the_restatement():
    """What the counters of the degenerate cases must be, written down."""
    want = {'zero_length': [0, 0, 1, 0, 0], 'margin_ge_L': [0, 0, 2, 0, 0], 'range_zero': [0, 0, 1, 0, 0], 'steps1': [1, 0, 0, 1, 1], 'steps5': [1, 0, 0, 1, 5],
            'steps_exact': [1, 0, 0, 0, 12], 'range_cut': [1, 0, 0, 0, 4], 'bad_origin_alone': [0, 1, 0, 0, 0], 'all_moving': [0, 0, 4, 0, 0], 'n0': [0] * 5}
    for name, counters in want.items():
        assert _restate(CASES[name])[1] == counters, name
    for name in ('bad_first', 'bad_last'):
        assert _restate(CASES[name])[1][:4] == [4, 5, 0, 0], name
    for j in range(5):
        assert _restate(CASES['bad_alone%d' % j]) == ({}, [0, 1, 0, 0, 0])
    assert _restate(CASES['bad_origins'])[1][:3] == [1, 4, 0] and _restate(CASES['bad_index'])[1][:3] == [2, 2, 0]
    assert _restate(CASES['some_moving'])[1][:3] == [2, 1, 2]                   # the moving point with a NaN is dropped, not skipped: the drop rule comes first
    pierced, counters = _restate(CASES['m0'])
    assert pierced == {} and counters[0] == 4 and counters[4] == 0
    walks = []
    _restate(CASES['steps5'], walks)
    assert walks[0][1] == [(k, 0, 0) for k in range(5)]                          # the visits made before the cut are kept


def test_index_bound_and_decoys():
    """Rays that end in the last voxel of an axis walk its last three voxels and stop; a ray that ends outside is dropped; no decoy is touched."""
    walked, decoys = ah.walked_voxels()
    pierced, counters = _restate(CASES['bound'])
    assert counters == [6, 2, 0, 0, 18]
    assert pierced == {v: 1 for v in walked}
    assert all(d not in pierced for d in decoys)


def test_stamp_rule_at_equality():
    """Voxel k holds (t_first, t_last) = (3, 3 + k).  A row counts iff t_last < s or t_first > s."""
    want = {None: [1, 1, 1, 1], 2: [1, 1, 1, 1], 3: [0, 0, 0, 0], 4: [1, 0, 0, 0], 5: [1, 1, 0, 0], 6: [1, 1, 1, 0], 7: [1, 1, 1, 1]}
    for s, row in want.items():
        pierced, counters = _restate(CASES['stamp_%s' % s])
        assert [pierced.get((k, 0, 0), 0) for k in range(4)] == row, s
        assert counters == [1, 0, 0, 0, sum(row)]


def _slab(o, d, lo, hi, t_end):
    """Chord of the segment o + t d, t in [0, t_end], inside the boxes [lo, hi] ([V,3] each): its length in t, negative where there is none."""
    t0, t1 = np.zeros(lo.shape[0]), np.full(lo.shape[0], t_end)
    with np.errstate(all='ignore'):
        for a in range(3):
            if d[a] == 0.0:
                out = (o[a] < lo[:, a]) | (o[a] > hi[:, a])
                t0, t1 = np.where(out, 1.0, t0), np.where(out, 0.0, t1)
            else:
                ta, tb = (lo[:, a] - o[a]) / d[a], (hi[:, a] - o[a]) / d[a]
                t0, t1 = np.maximum(t0, np.minimum(ta, tb)), np.minimum(t1, np.maximum(ta, tb))
    return t1 - t0


def test_walk_geometry_on_the_restatement():
    """The walk visits what the ray geometrically crosses.  Per ray of the random scene, cut at t_end, over the whole 40^3 block: every voxel whose box
    shrunk by 1e-9 m holds a chord longer than 1e-9 m is visited; every visited voxel's box grown by 1e-9 m is hit; visited voxels that meet only the
    second condition are 'in the band', at most 0.1 % of the must-visit pairs."""
    eps = 1e-9
    idx = ah.block(-20, 20)
    lo, hi = idx * 0.1, (idx + 1) * 0.1
    row_of = {tuple(c): j for j, c in enumerate(idx.tolist())}
    walks = []
    _restate(CASES['random'], walks)
    must_total = band = 0
    for n, visited, (o, d, L, t_end) in walks:
        o, d = np.array(o), np.array(d)
        must = _slab(o, d, lo + eps, hi - eps, t_end) * L > eps
        may = _slab(o, d, lo - eps, hi + eps, t_end) >= 0.0
        seen = np.zeros(idx.shape[0], bool)
        for c in visited:
            assert c in row_of, (n, c)                                           # the rays stay inside the block
            seen[row_of[c]] = True
        assert len(set(visited)) == len(visited), n
        assert not np.any(must & ~seen), (n, idx[must & ~seen][:4])
        assert not np.any(seen & ~may), (n, idx[seen & ~may][:4])
        must_total += int(must.sum())
        band += int((seen & ~must).sum())
    assert must_total > 5000 and band <= 0.001 * must_total, (must_total, band)


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_pierce_workspace_bytes', 'pcacc_accum_pierce'):
        assert ('int %s(' % name) in header
        assert name in native.EXPORTS
    assert ' C7. ' in header
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_pierce.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_grid.h"']
    assert callable(native.accum_pierce)
    cpu = AccumulatedCloud(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.see_through(torch.zeros(4, 3), np.zeros(3))
    with pytest.raises(native.NativeError):
        cpu.pierced()
    cpu_tables = (torch.zeros(4, dtype=torch.int64), torch.zeros(5, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(native.NativeError):
        native.accum_pierce(torch.zeros(4, 3), None, torch.zeros(1, 3, dtype=torch.float64), None, None, 0.1, 0.2, None, None, 4096, cpu_tables, 0,
                            torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
_device_maps = {}


def _device_map(name, fresh=False, capacity=64):
    """A map on the device; the shared ones are never cleared: a test reads the sidecar before and after its call."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    if not fresh and name in _device_maps:
        return _device_maps[name]
    vs, adds = _map_adds(name)
    m = AccumulatedCloud(vs, DEV, capacity)
    for pts, stamp in adds:
        m.add(torch.from_numpy(pts).to(DEV), stamp=stamp)
    if not fresh:
        _device_maps[name] = m
    return m


def _see(m, case, **over):
    a = dict(case, **over)
    t = lambda v, dt=None: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dt)).to(DEV)
    return m.see_through(t(a['points'], np.float32).reshape(-1, 3), a['origins'], t(a.get('origin_index')), a.get('pose'), t(a.get('moving')),
                         a.get('stamp'), a.get('margin'), a.get('max_range'), a.get('max_steps', 4096))


def _delta(m, case):
    """What ONE call adds to the sidecar (key order) and to the counters."""
    before_p = m.pierced()
    before_c = m._pierce_counters.clone() if m._pierce_counters is not None else torch.zeros(5, dtype=torch.int64, device=DEV)
    after_c = _see(m, case)
    return m.pierced() - before_p, after_c - before_c


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """The same header, integers only: equal, on every scene of the CPU leg.  The map's records are not modified."""
    case = CASES[name]
    m = _device_map(case['map'])
    records = m.records()
    got_p, got_c = _delta(m, case)
    host_p, host_c, _ = _host(host_exe, tmp_path, case, name)
    assert got_p.dtype == torch.int32 and got_c.dtype == torch.int64 and got_c.is_cuda
    assert torch.equal(got_c.cpu(), torch.from_numpy(host_c.copy())), (name, got_c.tolist(), host_c.tolist())
    assert torch.equal(got_p.cpu(), torch.from_numpy(host_p.copy())), name
    for x, y, z in zip(m.records(), records, _ref_map(case['map'])[0].records()):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def _short_rays():
    rs = np.random.RandomState(12)
    origins = rs.uniform(-0.3, 0.3, (4, 3))
    return dict(map='third', points=rs.uniform(-0.9, 0.9, (70001, 3)).astype(np.float32), origins=origins,
                origin_index=rs.randint(0, 4, 70001).astype(np.int32), margin=0.1)


@pytest.mark.gpu
def test_kernel_on_70001_rays_gpu(host_exe, tmp_path):
    """More than one workgroup, n mod 64 != 0; two runs equal."""
    case = _short_rays()
    m = _device_map('third')
    got_p, got_c = _delta(m, case)
    host_p, host_c, visits = _host(host_exe, tmp_path, case, 'short70001')
    assert host_c[0] > 69000 and visits / host_c[0] < 60
    assert torch.equal(got_c.cpu(), torch.from_numpy(host_c.copy())) and torch.equal(got_p.cpu(), torch.from_numpy(host_p.copy()))
    again_p, again_c = _delta(m, case)
    assert torch.equal(again_p, got_p) and torch.equal(again_c, got_c)


@pytest.mark.gpu
def test_order_and_split_independence_gpu():
    """The result is a function of the SET of rays: shuffled and split over three calls, an equal sidecar and equal counters."""
    case = CASES['random']
    whole = _device_map('third', fresh=True)
    want_c = _see(whole, case)
    split = _device_map('third', fresh=True)
    perm = np.random.RandomState(13).permutation(400)
    for part in np.array_split(perm, 3):
        got_c = _see(split, case, points=case['points'][part], origin_index=case['origin_index'][part])
    assert torch.equal(split._pierced, whole._pierced) and torch.equal(got_c, want_c)
    assert whole.pierced().sum().item() == want_c[4].item() > 2000


def _check_sidecar(m, pierced, counters, what):
    coords = m.extract()['coords'].cpu().numpy()
    assert np.array_equal(m.pierced().cpu().numpy(), pref.aligned(pierced, coords)), what
    assert m._pierce_counters.tolist() == counters, what
    assert m._pierced.shape[0] == m.capacity == m._cur[0].shape[0] and int(m._pierced[m.num_voxels:].sum()) == 0, what


@pytest.mark.gpu
def test_add_carries_the_sidecar_gpu(tmp_path):
    """Pierce, add a window whose new voxels fall below, between and above the map, once more with growth 64 -> 4096 rows, pierce again: after every step
    the sidecar equals the restatement's dict, keyed by coordinates.  save / load mid-scene round-trips the sidecar and the counters."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    vs = 0.1
    first = ah.centres([(x, 0, 0) for x in range(0, 12, 2)] + [(x, 1, 0) for x in range(0, 12, 2)], vs)
    window = ah.centres([(-3, 0, 0), (-2, 5, 1)] + [(x, 0, 0) for x in range(1, 12, 2)] + [(20, 0, 0), (5, 0, 0), (14, -1, 2)], vs)
    big = ah.centres(ah.block(-7, 7)[::1], vs)[:2500]
    origins = np.array([[-0.55, 0.05, 0.05], [-0.55, 0.12, 0.03]])
    rays = dict(points=ah.centres([(13, 0, 0), (13, 1, 0), (25, 0, 0), (10, 1, 0), (-1, 6, 1)], vs), origins=origins, origin_index=np.array([0, 1, 0, 1, 0], np.int32),
                margin=0.0)
    m, r = AccumulatedCloud(vs, DEV, 64), ref.ReferenceMap(vs)
    pierced, counters = {}, [0] * 5

    def see(stamp):
        _see(m, rays, stamp=stamp)
        pref.pierce(pref.voxels_of(r), rays['points'], origins, rays['origin_index'], voxel_size=vs, margin=0.0, stamp=stamp, pierced=pierced, counters=counters)

    def add(pts, stamp):
        m.add(torch.from_numpy(pts).to(DEV), stamp=stamp)
        r.add(pts, stamp=stamp)

    add(first, 0)
    see(1)
    _check_sidecar(m, pierced, counters, 'pierced')
    assert counters[4] >= 10 and m.capacity == 64
    add(window, 1)
    _check_sidecar(m, pierced, counters, 'carried')
    keys = m.records()[0]
    old = set(ref.ReferenceMap(vs).add(first).rec)
    new = [k for k in keys.tolist() if k not in old]
    assert min(new) < min(old) and max(new) > max(old) and any(min(old) < k < max(old) for k in new)     # below, above and between
    see(2)
    _check_sidecar(m, pierced, counters, 'pierced again')
    path = str(tmp_path / 'mid.npz')
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(['keys', 'acc', 'stamps', 'voxel_size', 'dropped', 'pierced', 'pierce_counters'])
    loaded = AccumulatedCloud.load(path, DEV)
    _check_sidecar(loaded, pierced, counters, 'loaded')
    add(big, 2)
    assert m.capacity == 4096 and m.num_voxels > 2048
    _check_sidecar(m, pierced, counters, 'grown')
    loaded.add(torch.from_numpy(big).to(DEV), stamp=2)
    see(3)
    _check_sidecar(m, pierced, counters, 'pierced after growth')
    _see(loaded, rays, stamp=3)
    _check_sidecar(loaded, pierced, counters, 'loaded, continued')
    assert sum(pierced.values()) == counters[4] > 40
    m.clear()
    assert m._pierced is None and m.pierced().shape == (0,)
    m.add(torch.from_numpy(first).to(DEV))
    assert m._pierced is None and int(m.pierced().sum()) == 0 and m.pierced().shape == (12,)


@pytest.mark.gpu
def test_never_pierced_map_saves_what_it_saved_gpu(tmp_path):
    m = _device_map('slab', fresh=True)
    path = str(tmp_path / 'plain.npz')
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(['keys', 'acc', 'stamps', 'voxel_size', 'dropped'])
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    loaded = AccumulatedCloud.load(path, DEV)
    assert loaded._pierced is None and loaded._pierce_counters is None


def _read_ply_names(path):
    raw = open(path, 'rb').read()
    head = raw[:raw.index(b'end_header\n')].decode('ascii').split('\n')
    return [l.split()[2] for l in head if l.startswith('property ')]


@pytest.mark.gpu
def test_pierced_aligns_with_extract_and_save_ply_gpu(tmp_path):
    """pierced() under four filters, one of which keeps nothing; the PLY column exists iff a sidecar does."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    vs = 0.1
    rs = np.random.RandomState(14)
    pts = rs.uniform(-1, 1, (6000, 3)).astype(np.float32)
    mv = rs.uniform(0, 1, 6000) < 0.1
    m, r = AccumulatedCloud(vs, DEV, 64), ref.ReferenceMap(vs)
    m.add(torch.from_numpy(pts).to(DEV), None, torch.from_numpy(mv).to(DEV), 0)
    r.add(pts, None, mv, 0)
    path = str(tmp_path / 'a.ply')
    m.save_ply(path)
    assert 'pierced' not in _read_ply_names(path)
    assert m.pierced().dtype == torch.int32 and int(m.pierced().sum()) == 0 and m.pierced().shape[0] == m.num_voxels      # all zeros before any see_through
    rays = dict(points=rs.uniform(-1.3, 1.3, (300, 3)).astype(np.float32), origins=np.array([[0.01, 0.02, 0.03]]), margin=0.1)
    _see(m, rays, stamp=1)
    pierced, counters = pref.pierce(pref.voxels_of(r), rays['points'], rays['origins'], voxel_size=vs, margin=0.1, stamp=1)
    kept = []
    for f in (dict(), dict(min_count=2, max_moving_fraction=0.0), dict(min_count=3), dict(min_count=10 ** 6)):
        cloud, got = m.extract(**f), m.pierced(**f)
        assert got.dtype == torch.int32 and got.shape[0] == cloud['count'].shape[0]
        assert np.array_equal(got.cpu().numpy(), pref.aligned(pierced, cloud['coords'].cpu().numpy())), f
        kept.append(got.shape[0])
    assert kept[0] == m.num_voxels > kept[1] > 0 and kept[2] > 0 and kept[3] == 0 and counters[4] > 500
    f = dict(min_count=2, max_moving_fraction=0.0)
    m.save_ply(path, **f)
    assert _read_ply_names(path)[-5:] == ['count', 'moving', 't_first', 't_last', 'pierced']
    raw = open(path, 'rb').read()
    v = m.pierced(**f).shape[0]
    row = np.dtype([(n, '<f4') for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')] + [(n, '<i4') for n in ('count', 'moving', 't_first', 't_last', 'pierced')])
    body = np.frombuffer(raw, row, v, raw.index(b'end_header\n') + len(b'end_header\n'))
    assert np.array_equal(body['pierced'], m.pierced(**f).cpu().numpy())


# ---- the capability: a ghost trail that only the rays reveal -------------------------------------------------------------------------------
def _ghost_restatement():
    vs = 0.1
    r = ref.ReferenceMap(vs)
    pierced, counters = {}, [0] * 5
    for k, (wall, cluster, _) in enumerate(ah.ghost_scans()):
        pts = np.concatenate([wall, cluster])
        pref.pierce(pref.voxels_of(r), pts, ah.GHOST_SENSOR, voxel_size=vs, stamp=k, pierced=pierced, counters=counters)
        r.add(pts, stamp=k)
    return r, pierced, counters


def test_ghost_scene_in_the_restatement():
    """On the CPU, before a GPU is involved: no wall voxel is ever pierced (end points mid-layer, margin 2 voxels, incidence below 45 degrees), and every
    cluster voxel of stamps 0-4 that a later wall ray geometrically crosses (slab test, a chord of more than 1e-9 m inside the box shrunk by 1e-9 m,
    the ray cut at its t_end) has a count of at least 1."""
    vs, eps = 0.1, 1e-9
    scans = ah.ghost_scans()
    r, pierced, counters = _ghost_restatement()
    assert counters[1] == counters[2] == counters[3] == 0
    wall_vox = {(30, y, z) for y in range(-20, 20) for z in range(-10, 10)}
    assert wall_vox <= set(pref.voxels_of(r)) and all(pierced.get(v, 0) == 0 for v in wall_vox)
    crossed_total = 0
    for j in range(5):
        vox = np.array(scans[j][2])
        lo, hi = vox * vs + eps, (vox + 1) * vs - eps
        crossed = np.zeros(len(vox), bool)
        for k in range(j + 1, 6):
            for p in scans[k][0].astype(np.float64):
                d = p - ah.GHOST_SENSOR[0]
                L = float(np.sqrt((d * d).sum()))
                crossed |= _slab(ah.GHOST_SENSOR[0], d, lo, hi, 1.0 - 0.2 / L) * L > eps
        assert crossed.sum() >= 9, (j, crossed.sum())
        assert all(pierced.get(tuple(v), 0) >= 1 for v in vox[crossed].tolist()), j
        crossed_total += int(crossed.sum())
    assert crossed_total >= 100


@pytest.mark.gpu
def test_ghost_scene_gpu():
    """see_through(stamp=k) then add(stamp=k), six scans: the sidecar equals the restatement's, and `pierced() < 1` keeps the whole wall and removes the
    trail that the moving flag did not."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    r, pierced, counters = _ghost_restatement()
    m = AccumulatedCloud(0.1, DEV, 64)
    for k, (wall, cluster, _) in enumerate(ah.ghost_scans()):
        pts = torch.from_numpy(np.concatenate([wall, cluster])).to(DEV)
        got = m.see_through(pts, ah.GHOST_SENSOR, stamp=k)
        m.add(pts, stamp=k)
    assert got.tolist() == counters
    _check_sidecar(m, pierced, counters, 'ghost')
    cloud = m.extract(max_moving_fraction=0.0)
    assert cloud['count'].shape[0] == m.num_voxels                               # the moving flag alone keeps every ghost
    keep = (m.pierced(max_moving_fraction=0.0) < 1).cpu().numpy()
    coords = cloud['coords'].cpu().numpy()
    is_wall = coords[:, 0] == 30
    assert is_wall.sum() == 800 and keep[is_wall].all()
    early = ~is_wall & (cloud['t_last'].cpu().numpy() < 5)
    assert early.sum() == 5 * 27 and (~keep[early]).sum() >= 100


@pytest.mark.gpu
def test_see_through_results_on_the_model_forward_gpu(golden):
    """see_through_results on the model_tiny_test forward: walked + dropped + skipped = n, and the result equals a direct see_through with hand-built
    origins.  Nothing more is claimed: its frames are independent random clouds."""
    from helpers import make_batch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    from pcaccumulation_amd.motionnet import MotionNet
    from pcaccumulation_amd.synthetic import fill_state_dict_
    dev = torch.device(DEV)
    g = golden('model_tiny_test')
    cfg = default_config('waymo', 'test', n_sweeps=3, xy_range=8)
    inp = make_batch(cfg, [int(s) for s in g['seeds']], int(g['n_frames']), int(g['pts_per_frame']))
    model = MotionNet(cfg)
    fill_state_dict_(model)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in zip(g['tweak_keys'], g['tweak_vals']):
            sd[str(k)] += torch.from_numpy(v)
        sd['motionhead.mos_seg.seg_head.3.bias'] += torch.tensor([0.0, float(g['mos_shift'])])
    model = model.to(dev).eval().channels_last_()
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    torch.manual_seed(int(g['fwd_seed']))
    with torch.no_grad():
        out = model(inp)
    n = out['rec_est'].shape[0]
    offset = (0.5, -0.25, 1.75)
    a = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, stamp=0)
    b = AccumulatedCloud(0.2, dev, 64).add_results(out, inp, stamp=0)
    got = a.see_through_results(out, inp, sensor_offset=offset, stamp=1, max_range=6.0)
    ego = out['ego_motion_est'][0].cpu().numpy().astype(np.float64)
    origins = ((ego[:, :3, 0] * offset[0] + ego[:, :3, 1] * offset[1]) + ego[:, :3, 2] * offset[2]) + ego[:, :3, 3]
    same = b.see_through(out['rec_est'], origins, inp['time_indice'][:, 1], None, out['mos_est'].argmax(1) == 1, stamp=1, max_range=6.0)
    assert torch.equal(got, same) and torch.equal(a._pierced, b._pierced)
    assert int(got[0] + got[1] + got[2]) == n and int(got[0]) > 0 and int(a.pierced().sum()) == int(got[4])
    with pytest.raises(ValueError):
        a.see_through_results(dict(out, _n_batches=2), inp)


@pytest.mark.gpu
def test_argument_checks_gpu():
    from pcaccumulation_amd import native
    m = _device_map('slab', fresh=True)
    pts = torch.zeros(4, 3, device=DEV)
    o = np.zeros(3)
    with pytest.raises(native.NativeError):
        m.see_through(pts.cpu(), o)
    with pytest.raises(native.NativeError):
        m.see_through(pts, o, moving=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(native.NativeError):
        m.see_through(pts, o, origin_index=torch.zeros(4, dtype=torch.int32))
    for bad in (dict(points=torch.zeros(4, 2, device=DEV)), dict(origins=np.zeros((2, 2))), dict(origins=np.zeros((0, 3))), dict(origins=np.zeros((1, 3, 1))),
                dict(moving=torch.zeros(3, dtype=torch.bool, device=DEV)), dict(origin_index=torch.zeros(5, dtype=torch.int32, device=DEV)),
                dict(margin=-0.1), dict(margin=NAN), dict(margin=INF), dict(max_range=-1.0), dict(max_range=NAN), dict(max_steps=0),
                dict(max_steps=(1 << 16) + 1), dict(pose=np.eye(3))):
        with pytest.raises(ValueError):
            m.see_through(**dict(dict(points=pts, origins=o), **bad))
    assert m._pierced is None                                                    # nothing was launched, nothing allocated
    # the entry point itself: PCACC_E_ARG
    pierced, counters = torch.zeros(m.capacity, dtype=torch.int32, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV)
    org = torch.zeros(1, 3, dtype=torch.float64, device=DEV)
    good = dict(points=pts, moving=None, origins=org, origin_index=None, pose=None, voxel_size=0.1, margin=0.2, max_range=None, stamp=None, max_steps=4096,
                tables=m._cur, m=m.num_voxels, pierced=pierced, counters=counters)
    for bad in (dict(m=m.capacity + 1), dict(m=-1), dict(margin=-1.0), dict(margin=INF), dict(max_steps=0), dict(max_steps=(1 << 16) + 1),
                dict(voxel_size=0.0), dict(voxel_size=INF), dict(origins=torch.zeros(0, 3, dtype=torch.float64, device=DEV))):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_pierce(**dict(good, **bad))
    assert int(pierced.sum()) == 0 and int(counters.sum()) == 0
    native.accum_pierce(**good)
    assert counters.tolist() == [0, 0, 4, 0, 0]                                  # four zero-length rays
    # an int64 origin row that would wrap to a valid int32 row is still outside [0, S): dropped
    rows = torch.tensor([1 << 32, 0, -(1 << 32), 1], dtype=torch.int64, device=DEV)
    got = m.see_through(torch.from_numpy(CASES['bad_index']['points']).to(DEV), np.full((2, 3), 0.05), origin_index=rows)
    assert got.tolist()[:4] == [2, 2, 0, 0]
