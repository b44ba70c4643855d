"""Observed space (include/pcacc.h C14): ObservedSpace.observe / observe_results / extract / lookup / lookup_voxels / occupancy /
forget / save / load.

CPU leg: csrc/accum_observe.h -- the code the kernels run -- built with g++ (-ffp-contract=off, every index assert-checked, poison behind the last row and
the last visit, C7's walk asserted equal visit for visit) against the plain-Python restatement tests/accumulate_observe_reference.py (a dict of
coordinates, no keys, no sort): every record, counter and state word EQUAL, on C7's scenes, on a second and third call, on lookups and on the two
"does not fit" answers; the figures of the scenes checked on the restatement alone.
GPU leg: the kernels against the host build, integer for integer; the set property; growth and the visit budget; the two "does not fit" answers by
snapshot; lookup, occupancy, forget, save / load; the capability -- what is gone against what was never looked at; the model tie-in.
Every result is an integer: no test has a tolerance."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_observe_reference as oref
import test_accumulate_pierce as c7
from accumulate_helpers import DEV, EDGE
from helpers import ROOT
from pcaccumulation_amd.config import default_config

NAN, INF = float('nan'), float('inf')
STATE_WORDS = 16
NUM_VOXELS, STATUS, NEEDED, NEEDED_VISITS, CALL_VISITS, CALL_VOXELS, WALKED = 0, 1, 2, 3, 4, 5, 6
OK, TOO_SMALL, BAD_STATE, TOO_MANY = 0, 1, 2, 3
_ARGS = ('origin_index', 'pose', 'moving', 'stamp', 'margin', 'max_range', 'max_steps')
_VOXEL_SIZE = {'third': 0.1, 'block9': 0.25, 'slab': 0.1, 'bound': 0.01}           # of the maps C7's cases were written for


# ---- calls: the arguments of ONE observe ------------------------------------------------------------------------------------------------------------
def _calls():
    """C7's cases (tests/test_accumulate_pierce.py) without their maps: random, ties, face, the degenerate rays, the non-finite points and origins, the
    origin rows outside the table, all moving, n = 0, the index bound, the ray counts around the wave size."""
    calls = {}
    for name, case in c7.CASES.items():
        if name.startswith('stamp_') or name == 'm0':                            # the stamp rule and the empty map are C7's own
            continue
        call = {k: case[k] for k in ('points', 'origins') + _ARGS if k in case and k != 'stamp'}
        call['vs'] = _VOXEL_SIZE[case['map']]
        calls[name] = call
    return calls


CALLS = _calls()
CALL_NAMES = sorted(CALLS)


def _sequence():
    """Three calls on one table at 0.1 m: the random rays at stamp 5; 200 of them again, in another order, at the lower stamp 3 (every voxel is in the
    table); rays 60 m away on either side at the higher stamp 9 (every voxel falls below the table's first key or above its last)."""
    pts, origins, index = ah.random_rays()
    first = dict(vs=0.1, points=pts, origins=origins, origin_index=index, margin=0.2, stamp=5)
    part = np.random.RandomState(3).permutation(400)[:200]
    second = dict(first, points=pts[part], origin_index=index[part], stamp=3)
    rs = np.random.RandomState(4)
    far = np.array([[-60.03, 0.02, 0.01], [60.03, 0.02, 0.01]])
    side = rs.randint(0, 2, 80).astype(np.int32)
    third = dict(vs=0.1, points=(far[side] + rs.uniform(-1, 1, (80, 3))).astype(np.float32), origins=far, origin_index=side, margin=0.2, stamp=9)
    return [first, second, third]


def _short_rays():
    rs = np.random.RandomState(12)
    return dict(vs=0.1, points=rs.uniform(-0.45, 0.45, (70001, 3)).astype(np.float32), origins=rs.uniform(-0.3, 0.3, (4, 3)),
                origin_index=rs.randint(0, 4, 70001).astype(np.int32), margin=0.1)


# ---- the capability scene ------------------------------------------------------------------------------------------------------------------------------
WALL = [(30, y, z) for y in range(-20, 20) for z in range(-10, 10)]
CLUSTER_K = [(15 + a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
CLUSTER_U = [(15 + a, 14 + b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
WALL_CALL = dict(vs=0.1, points=ah.centres(WALL, 0.1), origins=ah.GHOST_SENSOR, margin=0.2)


def _restate(call, space=None, per_ray=None):
    space = oref.ReferenceSpace(call['vs']) if space is None else space
    return space.observe(call['points'], call['origins'], per_ray=per_ray, **{k: call[k] for k in _ARGS if k in call})


_restated = {}


def _restated_call(name):
    """The restatement of one named call on an empty table, computed once and never modified."""
    if name not in _restated:
        _restated[name] = _restate(WALL_CALL if name == 'wall' else CALLS[name])
    return _restated[name]


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_observe_host_driver', 'acco')
EMPTY = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((2, 0), np.int32))
_host_cache = {}


def _host(exe, tmp_path, tag, call, table=EMPTY, state=None, out_capacity=None, visit_capacity=1 << 16, spare=3, lookup=None, cache=True):
    """The g++ build of accum_observe.h on one call and one lookup (every assert of the driver aborts it).  table = (keys, rays, stamps [2,m]) before the
    call; lookup = dict(points= or coords=, pose=, min_rays=).  -> dict(state [16], call [5], keys, rays, stamps: the table the call leaves, l_status,
    l_rays, l_stamps [2,n], l_counters [4]: the lookup on that table)."""
    if cache and tag in _host_cache:
        return _host_cache[tag]
    keys, rays, stamps = table
    m = keys.shape[0]
    pts = np.ascontiguousarray(call['points'], np.float32).reshape(-1, 3)
    n = pts.shape[0]
    org = np.ascontiguousarray(call['origins'], np.float64).reshape(-1, 3)
    mv, idx, pose, max_range = call.get('moving'), call.get('origin_index'), call.get('pose'), call.get('max_range')
    margin = call['margin'] if call.get('margin') is not None else 2.0 * call['vs']
    if state is None:
        state = np.zeros(STATE_WORDS, np.int64)
        state[NUM_VOXELS] = m
    look = dict(lookup or {})
    coords = look.get('coords')
    rows = np.zeros((0, 3), np.float32) if not look else (np.ascontiguousarray(look['points'], np.float32).reshape(-1, 3) if coords is None
                                                         else np.ascontiguousarray(coords, np.int32).reshape(-1, 3))
    head = [n, org.shape[0], m, m + spare, m + visit_capacity if out_capacity is None else out_capacity, visit_capacity, call.get('stamp', 0),
            call.get('max_steps', 4096), mv is not None, idx is not None, pose is not None, max_range is not None, rows.shape[0], coords is not None,
            look.get('min_rays', 1), look.get('pose') is not None]
    raw = ah.run_driver(exe, tmp_path, tag, np.array(head, np.int64), np.array([call['vs'], margin, 0.0 if max_range is None else max_range], np.float64),
                        pts, np.zeros(n, np.uint8) if mv is None else np.asarray(mv).astype(np.uint8), org,
                        np.zeros(n, np.int32) if idx is None else np.asarray(idx, np.int32), np.eye(4) if pose is None else np.ascontiguousarray(pose, np.float64),
                        np.ascontiguousarray(keys, np.int64), np.ascontiguousarray(rays, np.int64), np.ascontiguousarray(stamps, np.int32),
                        np.ascontiguousarray(state, np.int64), rows, np.eye(4) if look.get('pose') is None else np.ascontiguousarray(look['pose'], np.float64),
                        suffix='.bin')
    out, off = ah.unpack(raw, 0, [('state', np.int64, (STATE_WORDS,)), ('call', np.int64, (5,)), ('rows', np.int64, (1,))])
    r, nl = int(out['rows'][0]), rows.shape[0]
    more, off = ah.unpack(raw, off, [('keys', np.int64, (r,)), ('rays', np.int64, (r,)), ('stamps', np.int32, (2, r)), ('l_status', np.uint8, (nl,)),
                                     ('l_rays', np.int64, (nl,)), ('l_stamps', np.int32, (2, nl)), ('l_counters', np.int64, (4,))])
    assert off == len(raw)
    out.update(more)
    assert np.all(out['keys'][1:] > out['keys'][:-1])
    if cache:
        _host_cache[tag] = out
    return out


def _table(h):
    return h['keys'], h['rays'], h['stamps']


def _assert_host_is(h, space, what):
    """The driver's table and cumulative counters are the restatement's, record for record."""
    assert oref.table_of(h['keys'], h['rays'], h['stamps']) == space.rec, what
    assert h['keys'].shape[0] == len(space.rec) == h['state'][NUM_VOXELS], what
    assert h['state'][WALKED:WALKED + 5].tolist() == space.counters, (what, h['state'].tolist(), space.counters)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------------
def test_random_scene_figures_in_the_restatement():
    """What the issue states about the random rays at 0.1 m with margin 0.2, on the restatement alone."""
    per_ray = []
    space = _restate(CALLS['random'], per_ray=per_ray)
    assert sum(space.counters[:3]) == 400 and space.counters[oref.VISITS] == 10907 == sum(per_ray)
    assert len(space.rec) == 6762 and max(r[0] for r in space.rec.values()) == 147
    assert sum(r[0] for r in space.rec.values()) == 10907                        # one ray visits a voxel at most once
    assert all(r[1] == r[2] == 0 for r in space.rec.values())


@pytest.mark.parametrize('name', CALL_NAMES)
def test_host_build_equals_the_restatement(host_exe, tmp_path, name):
    """One call on an empty table: every record, the five counters and the state words."""
    call = CALLS[name]
    space = _restated_call(name)
    h = _host(host_exe, tmp_path, name, call)
    _assert_host_is(h, space, name)
    n = np.asarray(call['points']).reshape(-1, 3).shape[0]
    assert sum(space.counters[:3]) == n and h['call'].tolist() == space.counters
    assert h['state'][STATUS] == OK and h['state'][CALL_VISITS] == space.counters[oref.VISITS] and h['state'][CALL_VOXELS] == len(space.rec)
    assert h['state'][NEEDED] == len(space.rec)


def test_visited_lists_and_degenerate_rays_in_the_restatement():
    """C7's literal walks, now as table rows: the visited list of `ties` written down, the start voxel included, whether or not a cloud keeps it."""
    ties = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    assert _restated_call('ties').rec == {c: [1, 0, 0] for c in ties} and _restated_call('ties').counters == [1, 0, 0, 0, 10]
    assert _restated_call('face').rec == {(k, 1, 1): [1, 0, 0] for k in range(2, -4, -1)}
    want = {'zero_length': [0, 0, 1, 0, 0], 'margin_ge_L': [0, 0, 2, 0, 0], 'range_zero': [0, 0, 1, 0, 0], 'steps1': [1, 0, 0, 1, 1], 'steps5': [1, 0, 0, 1, 5],
            'steps_exact': [1, 0, 0, 0, 12], 'range_cut': [1, 0, 0, 0, 4], 'bad_origin_alone': [0, 1, 0, 0, 0], 'all_moving': [0, 0, 4, 0, 0], 'n0': [0] * 5}
    for name, counters in want.items():
        assert _restated_call(name).counters == counters, name
        assert sum(r[0] for r in _restated_call(name).rec.values()) == counters[4], name
    assert _restated_call('steps5').rec == {(k, 0, 0): [1, 0, 0] for k in range(5)}
    for name in ('bad_first', 'bad_last'):
        assert _restated_call(name).counters[:4] == [4, 5, 0, 0], name
    for j in range(5):
        assert _restated_call('bad_alone%d' % j).rec == {} and _restated_call('bad_alone%d' % j).counters == [0, 1, 0, 0, 0]
    assert _restated_call('bad_origins').counters[:3] == [1, 4, 0] and _restated_call('bad_index').counters[:3] == [2, 2, 0]
    assert _restated_call('some_moving').counters[:3] == [2, 1, 2]
    walked, decoys = ah.walked_voxels()
    bound = _restated_call('bound')
    assert bound.counters == [6, 2, 0, 0, 18] and bound.rec == {v: [1, 0, 0] for v in walked} and not set(decoys) & set(bound.rec)


def test_second_and_third_call(host_exe, tmp_path):
    """A call that overlaps the table at a lower stamp, then one that falls wholly below and above it at a higher stamp: host build == restatement after
    every call, and the stamps are the minimum and maximum of the calls that visited the voxel."""
    calls = _sequence()
    space = oref.ReferenceSpace(0.1)
    table, state = EMPTY, None
    sizes = []
    for k, call in enumerate(calls):
        before = dict((c, list(r)) for c, r in space.rec.items())
        _restate(call, space)
        h = _host(host_exe, tmp_path, 'seq%d' % k, call, table, state)
        _assert_host_is(h, space, k)
        table, state = _table(h), h['state']
        sizes.append((len(before), len(space.rec), before))
    assert sizes[0][:2] == (0, 6762) and sizes[1][:2] == (6762, 6762) and sizes[2][1] > 6762 + 100
    after_second = sizes[2][2]
    assert {(r[1], r[2]) for r in after_second.values()} == {(3, 5), (5, 5)}     # call 2 visits only voxels of call 1; none is new
    new = [c for c in space.rec if c not in after_second]
    assert all(space.rec[c][1:] == [9, 9] for c in new) and all(space.rec[c] == after_second[c] for c in after_second)
    old_keys = sorted(ah.key(c) for c in after_second)
    new_keys = [ah.key(c) for c in new]
    assert min(new_keys) < old_keys[0] and max(new_keys) > old_keys[-1] and not any(old_keys[0] < k < old_keys[-1] for k in new_keys)


def test_does_not_fit_answers_in_the_host_build(host_exe, tmp_path):
    """TOO_SMALL and TOO_MANY exactly at the bound, and one below it: the table, NUM_VOXELS and the cumulative counters stay."""
    first, second, _ = _sequence()
    assert _host(host_exe, tmp_path, 'fit', first, out_capacity=6762, visit_capacity=10907, cache=False)['state'][STATUS] == OK
    h = _host(host_exe, tmp_path, 'small', first, out_capacity=6761, visit_capacity=10907, cache=False)
    assert h['state'][[NUM_VOXELS, STATUS, NEEDED]].tolist() == [0, TOO_SMALL, 6762] and h['keys'].shape[0] == 0 and not h['state'][WALKED:WALKED + 5].any()
    h = _host(host_exe, tmp_path, 'many', first, visit_capacity=10906, cache=False)
    assert h['state'][[NUM_VOXELS, STATUS, NEEDED_VISITS]].tolist() == [0, TOO_MANY, 10907] and h['keys'].shape[0] == 0 and not h['state'][WALKED:WALKED + 5].any()
    base = _host(host_exe, tmp_path, 'seq0', first)
    far = _sequence()[2]
    for tag, kw, status in (('small2', dict(out_capacity=6762), TOO_SMALL), ('many2', dict(visit_capacity=100), TOO_MANY)):
        h = _host(host_exe, tmp_path, tag, far, _table(base), base['state'], cache=False, **kw)
        assert h['state'][STATUS] == status and h['state'][NUM_VOXELS] == 6762
        assert np.array_equal(h['state'][WALKED:WALKED + 5], base['state'][WALKED:WALKED + 5])
        for f in ('keys', 'rays', 'stamps'):
            assert np.array_equal(h[f], base[f]), (tag, f)
    bad = base['state'].copy()
    bad[NUM_VOXELS] = 6762 + 4                                                   # more rows than the input table has room for (capacity m + 3)
    h = _host(host_exe, tmp_path, 'bad', second, _table(base), bad, cache=False)
    assert h['state'][STATUS] == BAD_STATE and h['state'][NUM_VOXELS] == 6762 + 4 and np.array_equal(h['keys'], base['keys'])


def _lookup_cases():
    """(call, lookup): seen, unseen and invalid points under a non-identity pose with min_rays at a voxel's count and one above; voxel rows at the index
    bound."""
    space = _restated_call('random')
    top = max(space.rec, key=lambda c: (space.rec[c][0], c))                      # 147 rays
    some = sorted(space.rec)[::400]
    pose = ah.rot_xyz(0.2, -0.1, 0.3, (0.4, -0.2, 0.1))
    inv = np.linalg.inv(pose)
    world = np.concatenate([ah.centres([top] + some, 0.1).astype(np.float64), [[5.05, 5.05, 5.05], [-7.25, 0.15, 3.35]]])
    scan = (world @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    scan = np.concatenate([scan, np.array([[NAN, 0, 0], [0, INF, 0], [40000, 0, 0]], np.float32)])
    cases = {'points147': (CALLS['random'], dict(points=scan, pose=pose, min_rays=147)), 'points148': (CALLS['random'], dict(points=scan, pose=pose, min_rays=148)),
             'points1': (CALLS['random'], dict(points=scan, pose=pose, min_rays=1))}
    coords = np.array([(-EDGE, 1, -2), (EDGE - 1, 1, -2), (EDGE, 1, -2), (1, -EDGE - 1, -2), (1, -2, EDGE - 3), (0, 0, 0), (-EDGE, 2, -2), (1, EDGE - 1, -2)],
                      np.int32)
    cases['coords'] = (CALLS['bound'], dict(coords=coords, min_rays=1))
    cases['coords2'] = (CALLS['bound'], dict(coords=coords, min_rays=2))
    return cases


LOOKUPS = _lookup_cases()


def _restated_lookup(name):
    call, look = LOOKUPS[name]
    space = _restated_call('random' if 'points' in look else 'bound')
    if 'points' in look:
        return space.lookup(look['points'], look['pose'], look['min_rays'])
    return space.lookup_voxels(look['coords'], look['min_rays'])


def _host_lookup(exe, tmp_path, name):
    call, look = LOOKUPS[name]
    return _host(exe, tmp_path, 'look_' + name, call, lookup=look)


@pytest.mark.parametrize('name', sorted(LOOKUPS))
def test_lookup_host_build_equals_the_restatement(host_exe, tmp_path, name):
    want = _restated_lookup(name)
    h = _host_lookup(host_exe, tmp_path, name)
    got = list(zip(h['l_status'].tolist(), h['l_rays'].tolist(), h['l_stamps'][0].tolist(), h['l_stamps'][1].tolist()))
    assert got == want, name
    status = np.array([w[0] for w in want])
    assert h['l_counters'].tolist() == [len(want), int((status & 1 != 0).sum()), int((status & 2 != 0).sum()), int((status & 4 != 0).sum())]


def test_lookup_cases_hold_what_they_are_meant_to():
    """Seen, unseen and invalid rows are all there; min_rays at the count keeps ENOUGH, one above drops it; the rows at -2^20 and 2^20 - 1 are seen, the
    row at 2^20 is invalid."""
    at, above, one = _restated_lookup('points147'), _restated_lookup('points148'), _restated_lookup('points1')
    assert at[0] == (7, 147, 0, 0) and above[0] == (3, 147, 0, 0)
    assert [w[0] for w in one[-5:]] == [1, 1, 0, 0, 0] and all(w[0] == 7 for w in one[:-5]) and len(one) >= 20
    rows = _restated_lookup('coords')
    assert [w[0] for w in rows] == [7, 7, 0, 0, 7, 1, 1, 7] and _restated_lookup('coords2')[0] == (3, 1, 0, 0)


def test_observe_chunks_stay_below_2_31():
    from pcaccumulation_amd.accumulate import _observe_chunks
    for n, max_steps in ((800000, 4096), (5, 65536), (1, 1), (0, 4096), (524288, 4096), (524287, 4096), (1 << 30, 65536 // 4096)):
        chunks = _observe_chunks(n, max_steps)
        assert all(0 < (hi - lo) * max_steps < (1 << 31) for lo, hi in chunks), (n, max_steps)
        assert [lo for lo, _ in chunks] == [0] * bool(n) + [hi for _, hi in chunks[:-1]] and (chunks[-1][1] if n else 0) == n
    assert len(_observe_chunks(800000, 4096)) == 2 and _observe_chunks(5, 65536) == [(0, 5)] and _observe_chunks(524287, 4096) == [(0, 524287)]


def _capability():
    """Session B's space on the restatement, and the visits of its rays."""
    per_ray = []
    return _restate(WALL_CALL, per_ray=per_ray), per_ray


def test_capability_scene_in_the_restatement():
    """The wall scene at 0.1 m, margin 0.2: 34 588 visits, at most 57 per ray, 7 518 voxels; every voxel of K is seen by at least 4 rays, none of U and
    none of the wall (the margin keeps rays off their own surface)."""
    space, per_ray = _capability()
    assert space.counters == [800, 0, 0, 0, 34588] and max(per_ray) == 57 and len(space.rec) == 7518
    assert all(space.rec[c][0] >= 4 for c in CLUSTER_K) and min(space.rec[c][0] for c in CLUSTER_K) == 4
    assert not any(c in space.rec for c in CLUSTER_U) and not any(c in space.rec for c in WALL)
    assert len(set(WALL) | set(CLUSTER_K) | set(CLUSTER_U)) == 854


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud, ObservedSpace
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_observe_workspace_bytes', 'pcacc_accum_observe', 'pcacc_accum_observed_lookup_workspace_bytes', 'pcacc_accum_observed_lookup'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C14. ' in header
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_observe.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_pierce.h"']
    assert (native.OBSERVED_VALID, native.OBSERVED_SEEN, native.OBSERVED_ENOUGH) == (oref.VALID, oref.SEEN, oref.ENOUGH)
    cpu = ObservedSpace(voxel_size=0.1, device='cpu', capacity=64)
    with pytest.raises(native.NativeError):
        cpu.observe(torch.zeros(4, 3), np.zeros(3))
    for call in (lambda: cpu.extract(), lambda: cpu.lookup(torch.zeros(4, 3)), lambda: cpu.lookup_voxels(torch.zeros(4, 3, dtype=torch.int32)),
                 lambda: cpu.forget(before_stamp=1)):
        with pytest.raises(native.NativeError):
            call()
    for bad in (dict(voxel_size=0.0), dict(voxel_size=INF), dict(capacity=0), dict(visit_budget=0), dict(visit_budget=1 << 31)):
        with pytest.raises(ValueError):
            ObservedSpace(**dict(dict(voxel_size=0.1, device='cpu'), **bad))
    with pytest.raises(ValueError):
        cpu.occupancy(AccumulatedCloud(0.2, 'cpu', 64), torch.zeros(1, 3, dtype=torch.int32))
    assert cpu.num_voxels == 0 and cpu.counters == dict(walked=0, dropped=0, skipped=0, truncated=0, visits=0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------
def _t(v, dtype=None):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype)).to(DEV)


def _observe(sp, call, **over):
    a = dict(call, **over)
    return sp.observe(_t(a['points'], np.float32).reshape(-1, 3), a['origins'], _t(a.get('origin_index')), a.get('pose'), _t(a.get('moving')), a.get('stamp', 0),
                      a.get('margin'), a.get('max_range'), a.get('max_steps', 4096))


def _space(vs, capacity=64, visit_budget=1 << 21):
    from pcaccumulation_amd.accumulate import ObservedSpace
    return ObservedSpace(vs, DEV, capacity, visit_budget)


def _columns(sp):
    """keys, rays, t_first, t_last of the rows in use, on the host."""
    sp._ensure()                                                                 # a space that has seen no ray yet has taken no memory
    n = sp.num_voxels
    keys, rays, stamps = sp._cur
    return [keys[:n].cpu(), rays[:n].cpu(), stamps[0, :n].cpu(), stamps[1, :n].cpu()]


def _assert_space_is_host(sp, h, what):
    want = [torch.from_numpy(h['keys']), torch.from_numpy(h['rays']), torch.from_numpy(h['stamps'][0].copy()), torch.from_numpy(h['stamps'][1].copy())]
    assert sp.num_voxels == h['keys'].shape[0], what
    for got, w in zip(_columns(sp), want):
        assert got.dtype == w.dtype and torch.equal(got, w), what
    assert list(sp.counters.values()) == h['state'][WALKED:WALKED + 5].tolist(), what
    assert sp._state[:1].tolist() == [sp.num_voxels] and sp._state[WALKED:WALKED + 5].tolist() == list(sp.counters.values()), what


def _assert_spaces_equal(a, b, what):
    assert a.num_voxels == b.num_voxels and a.counters == b.counters, what
    for x, y in zip(_columns(a), _columns(b)):
        assert torch.equal(x, y), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', CALL_NAMES)
def test_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """The same header, integers only: all four columns and the counters equal, on every scene of the CPU leg."""
    call = CALLS[name]
    sp = _observe(_space(call['vs']), call)
    _assert_space_is_host(sp, _host(host_exe, tmp_path, name, call), name)


@pytest.mark.gpu
def test_second_and_third_call_gpu(host_exe, tmp_path):
    sp = _space(0.1)
    table, state = EMPTY, None
    for k, call in enumerate(_sequence()):
        h = _host(host_exe, tmp_path, 'seq%d' % k, call, table, state)
        table, state = _table(h), h['state']
        _observe(sp, call)
        _assert_space_is_host(sp, h, k)


@pytest.mark.gpu
def test_kernel_on_70001_rays_gpu(host_exe, tmp_path):
    """More than one workgroup, n mod 64 != 0; two runs equal."""
    call = _short_rays()
    h = _host(host_exe, tmp_path, 'short70001', call, visit_capacity=1 << 20)
    assert h['state'][STATUS] == OK and h['state'][WALKED] > 69000 and h['state'][CALL_VISITS] > 200000
    sp = _observe(_space(0.1, 1 << 16), call)
    _assert_space_is_host(sp, h, 'short')
    _assert_spaces_equal(_observe(_space(0.1, 1 << 16), call), sp, 'again')


@pytest.mark.gpu
def test_set_property_gpu(host_exe, tmp_path):
    """Shuffled and split over three calls with one stamp; a visit budget that forces the TOO_MANY split; a capacity of 64 rows growing to fit 7 518:
    each the table of one plain call."""
    call = CALLS['random']
    whole = _observe(_space(0.1, 1 << 14), call)
    split = _space(0.1, 1 << 14)
    for part in np.array_split(np.random.RandomState(13).permutation(400), 3):
        _observe(split, call, points=call['points'][part], origin_index=call['origin_index'][part])
    _assert_spaces_equal(split, whole, 'split')
    wall = _observe(_space(0.1, 1 << 14), WALL_CALL)
    _assert_space_is_host(wall, _host(host_exe, tmp_path, 'wall', WALL_CALL), 'wall')
    assert wall.splits == 0 and wall.num_voxels == 7518 and wall.counters['visits'] == 34588
    tight = _observe(_space(0.1, 1 << 14, visit_budget=4096), WALL_CALL)          # 34 588 visits: nine pieces at least; visit_budget >= max_steps still holds
    assert tight.splits >= 1
    _assert_spaces_equal(tight, wall, 'budget')
    grown = _observe(_space(0.1, 64), WALL_CALL)
    assert grown.capacity == 8192 and grown._cur[0].shape[0] == 8192
    _assert_spaces_equal(grown, wall, 'grown')


def _native_observe(call, tables_in, m, tables_out, state, visit_capacity):
    from pcaccumulation_amd import native
    native.accum_observe(_t(call['points'], np.float32), None, _t(np.asarray(call['origins'], np.float64).reshape(-1, 3)), _t(call.get('origin_index')), None,
                         call.get('stamp', 0), call['vs'], call['margin'], None, 4096, visit_capacity, tables_in, m, tables_out, state)


@pytest.mark.gpu
def test_does_not_fit_answers_leave_everything_gpu(host_exe, tmp_path):
    """TOO_SMALL and TOO_MANY by snapshot, with a capacity and a budget the host build knows to be too small by one: the input tables, the poisoned output
    tables, NUM_VOXELS and the cumulative counters are what they were.  Nothing is overrun: the output tables are simply not written."""
    first, _, far = _sequence()
    base = _host(host_exe, tmp_path, 'seq0', first)
    after = _host(host_exe, tmp_path, 'seq_far', far, _table(base), base['state'])
    need_rows, need_visits = int(after['state'][NEEDED]), int(after['state'][CALL_VISITS])
    sp = _observe(_space(0.1, 1 << 14), first)
    _assert_space_is_host(sp, base, 'base')
    for what, rows, visits, status, word in (('small', need_rows - 1, need_visits, TOO_SMALL, NEEDED), ('many', need_rows, need_visits - 1, TOO_MANY, NEEDED_VISITS)):
        out = (torch.full((rows,), -77, dtype=torch.int64, device=DEV), torch.full((rows,), -78, dtype=torch.int64, device=DEV),
               torch.full((2, rows), -79, dtype=torch.int32, device=DEV))
        snap = [t.clone() for t in sp._cur] + [sp._state.clone()]
        _native_observe(far, sp._cur, sp.num_voxels, out, sp._state, visits)
        state = sp._state.tolist()
        assert state[STATUS] == status and state[word] == (need_rows if word == NEEDED else need_visits), (what, state)
        assert state[NUM_VOXELS] == 6762 and state[WALKED:WALKED + 5] == snap[3][WALKED:WALKED + 5].tolist(), what
        for got, want in zip(sp._cur, snap[:3]):
            assert torch.equal(got, want), what
        assert bool((out[0] == -77).all()) and bool((out[1] == -78).all()) and bool((out[2] == -79).all()), what
    out = (torch.empty((need_rows,), dtype=torch.int64, device=DEV), torch.empty((need_rows,), dtype=torch.int64, device=DEV),
           torch.empty((2, need_rows), dtype=torch.int32, device=DEV))
    _native_observe(far, sp._cur, sp.num_voxels, out, sp._state, need_visits)     # exactly enough of both: the call goes through
    assert sp._state.tolist()[:2] == [need_rows, OK] and torch.equal(out[0].cpu(), torch.from_numpy(after['keys']))
    assert torch.equal(out[1].cpu(), torch.from_numpy(after['rays'])) and torch.equal(out[2].cpu(), torch.from_numpy(after['stamps']))


_spaces = {}


def _shared_space(name):
    """A space after one named call; shared, never modified."""
    if name not in _spaces:
        call = WALL_CALL if name == 'wall' else CALLS[name]
        _spaces[name] = _observe(_space(call['vs'], 1 << 14), call)
    return _spaces[name]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(LOOKUPS))
def test_lookup_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """lookup and lookup_voxels: every output poisoned beforehand, every row written, equal to the host build; the wrapper returns the same."""
    from pcaccumulation_amd import native
    call, look = LOOKUPS[name]
    sp = _shared_space('random' if 'points' in look else 'bound')
    h = _host_lookup(host_exe, tmp_path, name)
    n = h['l_status'].shape[0]
    out = {'status': torch.full((n,), 0xa5, dtype=torch.uint8, device=DEV), 'rays': torch.full((n,), -0x5a5a5a5a5a5a5a5b, dtype=torch.int64, device=DEV),
           'stamps': torch.full((2, n), -0x5a5a5a5b, dtype=torch.int32, device=DEV)}
    counters = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    if 'points' in look:
        native.accum_observed_lookup(_t(look['points'], np.float32), None, _t(look['pose'], np.float64), sp.voxel_size, sp._cur, sp.num_voxels, look['min_rays'], out,
                                     counters)
        res = sp.lookup(_t(look['points'], np.float32), look['pose'], look['min_rays'])
    else:
        native.accum_observed_lookup(None, _t(look['coords'], np.int32), None, sp.voxel_size, sp._cur, sp.num_voxels, look['min_rays'], out, counters)
        res = sp.lookup_voxels(_t(look['coords'], np.int32), look['min_rays'])
    want = dict(status=h['l_status'], rays=h['l_rays'], t_first=h['l_stamps'][0].copy(), t_last=h['l_stamps'][1].copy(), counters=h['l_counters'])
    got = dict(status=out['status'], rays=out['rays'], t_first=out['stamps'][0], t_last=out['stamps'][1], counters=counters)
    for f, w in want.items():
        assert torch.equal(got[f].cpu(), torch.from_numpy(w)), (name, f)
        assert torch.equal(res[f].cpu(), torch.from_numpy(w)), (name, f, 'wrapper')


@pytest.mark.gpu
def test_lookup_of_nothing_and_in_nothing_gpu():
    """m = 0: every valid row is VALID alone; n = 0: empty columns and zero counters."""
    sp = _space(0.1)
    pts = _t(np.array([[0.05, 0.05, 0.05], [NAN, 0, 0]], np.float32))
    for res, want in ((sp.lookup(pts), [1, 0]), (sp.lookup_voxels(_t(np.array([[0, 0, 0], [EDGE, 0, 0]], np.int32))), [1, 0])):
        assert res['status'].tolist() == want and res['rays'].tolist() == [0, 0] and res['t_first'].tolist() == res['t_last'].tolist() == [0, 0]
        assert res['counters'].tolist() == [2, 1, 0, 0]
    full = _shared_space('random')
    for res in (full.lookup(torch.zeros(0, 3, device=DEV)), full.lookup_voxels(torch.zeros(0, 3, dtype=torch.int32, device=DEV))):
        assert res['status'].shape == res['rays'].shape == res['t_first'].shape == res['t_last'].shape == (0,) and res['counters'].tolist() == [0, 0, 0, 0]
    assert torch.equal(full.lookup_voxels(_t(np.array([[0, 0, 0], [1 << 40, 0, 0]], np.int64)))['status'].cpu() & 1, torch.tensor([1, 0], dtype=torch.uint8))


def _session_a():
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    a = AccumulatedCloud(0.1, DEV, 64)
    a.add(_t(ah.centres(WALL + CLUSTER_K + CLUSTER_U, 0.1)), stamp=0)
    return a


@pytest.mark.gpu
def test_occupancy_equals_the_restatement_gpu():
    """A cloud and a space under two filters, one of which turns OCCUPIED rows into FREE or UNKNOWN: a wall voxel and K get a second point each, so that
    min_count = 2 drops U and most of the wall from the cloud."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    space, _ = _capability()
    sp = _shared_space('wall')
    cloud = AccumulatedCloud(0.1, DEV, 64)
    cloud.add(_t(ah.centres(WALL + CLUSTER_K + CLUSTER_U, 0.1)), stamp=0)
    twice = WALL[:5] + CLUSTER_K
    cloud.add(_t(ah.centres(twice, 0.1)), stamp=1)
    rows = WALL[::7] + CLUSTER_K + CLUSTER_U + [(0, 0, 0), (5, 1, 0), (40, 0, 0), (EDGE - 1, 0, 0)]
    coords = np.array(rows + [(EDGE, 0, 0)], np.int64)
    seen = {}
    for f, occupied in ((dict(), set(WALL + CLUSTER_K + CLUSTER_U)), (dict(min_count=2), set(twice))):
        for min_rays in (1, 5, 801):
            got = sp.occupancy(cloud, _t(coords), min_rays=min_rays, **f)
            assert got.dtype == torch.uint8 and got.tolist() == space.occupancy(occupied, coords, min_rays), (f, min_rays)
            seen[(len(f), min_rays)] = got.tolist()
    plain, filtered = np.array(seen[(0, 1)]), np.array(seen[(1, 1)])
    assert set(plain[:len(rows) - 4]) == {oref.OCCUPIED} and set(filtered.tolist()) == {oref.UNKNOWN, oref.FREE, oref.OCCUPIED}
    assert ((plain == oref.OCCUPIED) & (filtered == oref.UNKNOWN)).any() and plain[-1] == oref.UNKNOWN and plain[-5] == oref.FREE
    assert seen[(0, 1)] != seen[(0, 801)]                                        # the sensor's own voxel: 800 rays
    assert sp.occupancy(cloud, torch.zeros(0, 3, dtype=torch.int32, device=DEV)).shape == (0,)
    with pytest.raises(ValueError):
        sp.occupancy(AccumulatedCloud(0.2, DEV, 64), _t(coords))
    with pytest.raises(TypeError):
        sp.occupancy(sp, _t(coords))


@pytest.mark.gpu
def test_forget_equals_the_restatement_gpu():
    """By stamp, by box and by both; the rows that stay keep their order and their records."""
    calls = _sequence()
    for kw in (dict(before_stamp=5), dict(before_stamp=6), dict(box=((-1.0, -0.55, -2.0), (0.95, 1.0, 0.349))), dict(before_stamp=4, box=((-70.0, -1, -1), (0.0, 1, 1))),
               dict(before_stamp=100), dict()):
        sp, space = _space(0.1, 1 << 14), oref.ReferenceSpace(0.1)
        for call in calls:
            _observe(sp, call)
            _restate(call, space)
        counters = sp.counters
        kept = sp.forget(**kw)
        assert kept == space.forget(**kw) == sp.num_voxels, kw
        keys, rays, stamps = sp.records()
        assert oref.table_of(keys, rays, stamps) == space.rec and np.all(keys[1:] > keys[:-1]), kw
        assert sp.counters == counters and sp._state.tolist()[NUM_VOXELS] == kept
        _observe(sp, calls[1])                                                   # the table goes on from what is left
        _restate(calls[1], space)
        assert oref.table_of(*sp.records()) == space.rec, kw
    assert kept == 6762 + len([c for c in space.rec if abs(c[0]) > 500])
    with pytest.raises(ValueError):
        sp.forget(box=((1, 0, 0), (0, 1, 1)))


@pytest.mark.gpu
def test_save_load_and_extract_gpu(tmp_path):
    """save / load mid-scene continues to the same table; extract(min_rays) against the restatement, and nothing above the maximum."""
    from pcaccumulation_amd.accumulate import ObservedSpace
    calls = _sequence()
    sp, straight = _space(0.1, 1 << 14), _space(0.1, 1 << 14)
    for call in calls:
        _observe(straight, call)
    _observe(sp, calls[0])
    path = str(tmp_path / 'space.npz')
    sp.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['counters', 'keys', 'rays', 'stamps', 'voxel_size']
        assert all(z[f].dtype.kind == 'i' for f in ('counters', 'keys', 'rays', 'stamps'))
    loaded = ObservedSpace.load(path, DEV)
    assert loaded.voxel_size == 0.1 and loaded.counters == sp.counters
    _assert_spaces_equal(loaded, sp, 'loaded')
    for call in calls[1:]:
        _observe(loaded, call)
    _assert_spaces_equal(loaded, straight, 'continued')
    space = oref.ReferenceSpace(0.1)
    for call in calls:
        _restate(call, space)
    top = max(r[0] for r in space.rec.values())
    for min_rays in (1, 3, top, top + 1):
        got = straight.extract(min_rays)
        want = sorted((c, r) for c, r in space.rec.items() if r[0] >= min_rays)
        assert got['coords'].dtype == torch.int32 and got['coords'].tolist() == [list(c) for c, _ in want], min_rays
        assert got['rays'].tolist() == [r[0] for _, r in want] and got['t_first'].tolist() == [r[1] for _, r in want]
        assert got['t_last'].tolist() == [r[2] for _, r in want]
        assert got['centers'].dtype == torch.float32 and np.array_equal(got['centers'].cpu().numpy(), ah.centres([c for c, _ in want], 0.1).reshape(-1, 3))
    assert straight.extract(top)['rays'].shape[0] >= 1 and straight.extract(top + 1)['rays'].shape[0] == 0
    straight.clear()
    assert straight.num_voxels == 0 and straight.extract()['rays'].shape[0] == 0 and sum(straight.counters.values()) == 0


@pytest.mark.gpu
def test_argument_checks_gpu():
    """Bad arguments raise before any launch: nothing is allocated."""
    from pcaccumulation_amd import native
    sp = _space(0.1, 64, visit_budget=4096)
    pts, o = torch.zeros(4, 3, device=DEV), np.zeros(3)
    with pytest.raises(native.NativeError):
        sp.observe(pts.cpu(), o)
    with pytest.raises(native.NativeError):
        sp.observe(pts, o, moving=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(native.NativeError):
        sp.observe(pts, o, origin_index=torch.zeros(4, dtype=torch.int32))
    for bad in (dict(points=torch.zeros(4, 2, device=DEV)), dict(origins=np.zeros((2, 2))), dict(origins=np.zeros((0, 3))),
                dict(moving=torch.zeros(3, dtype=torch.bool, device=DEV)), dict(origin_index=torch.zeros(5, dtype=torch.int32, device=DEV)),
                dict(margin=-0.1), dict(margin=NAN), dict(margin=INF), dict(max_range=-1.0), dict(max_range=NAN), dict(max_steps=0),
                dict(max_steps=(1 << 16) + 1), dict(max_steps=4097), dict(pose=np.eye(3)), dict(stamp=1 << 31)):
        with pytest.raises(ValueError):
            sp.observe(**dict(dict(points=pts, origins=o), **bad))
    assert sp._cur is None and sp._state is None                                 # nothing was launched, nothing allocated
    for call in (lambda: sp.lookup(pts, min_rays=0), lambda: sp.lookup(torch.zeros(4, 2, device=DEV)), lambda: sp.extract(0),
                 lambda: sp.lookup_voxels(torch.zeros(4, 3, device=DEV)), lambda: sp.forget(before_stamp=1 << 31), lambda: sp.forget(box=((0, 0), (1, 1)))):
        with pytest.raises(ValueError):
            call()
    # the entry point itself: PCACC_E_ARG, and the state words stay
    sp = _observe(_space(0.25, 64), CALLS['ties'])
    out = tuple(torch.empty_like(t) for t in sp._cur)
    org = torch.zeros(1, 3, dtype=torch.float64, device=DEV)
    good = dict(points=pts, moving=None, origins=org, origin_index=None, pose=None, stamp=0, voxel_size=0.25, margin=0.2, max_range=None, max_steps=4096,
                visit_capacity=1 << 14, tables_in=sp._cur, m=sp.num_voxels, tables_out=out, state=sp._state)
    state = sp._state.clone()
    for bad in (dict(margin=-1.0), dict(margin=INF), dict(max_steps=0), dict(max_steps=(1 << 16) + 1), dict(voxel_size=0.0), dict(voxel_size=INF),
                dict(visit_capacity=0), dict(visit_capacity=1 << 31), dict(max_range=-1.0), dict(tables_out=sp._cur),
                dict(tables_out=(out[0], sp._cur[1], out[2])), dict(origins=torch.zeros(0, 3, dtype=torch.float64, device=DEV)),
                dict(points=torch.zeros(1 << 15, 3, device=DEV), max_steps=1 << 16)):     # 2^15 rays of 2^16 steps: 2^31 possible visits
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_observe(**dict(good, **bad))
    assert torch.equal(sp._state, state)
    native.accum_observe(**good)
    assert sp._state.tolist()[:2] == [sp.num_voxels, OK] and sp._state.tolist()[WALKED:WALKED + 5] == [1, 0, 4, 0, 10]     # four zero-length rays
    for bad in (dict(m=65), dict(m=-1), dict(voxel_size=0.0)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_observed_lookup(**dict(dict(points=pts, coords=None, pose=None, voxel_size=0.1, tables=sp._cur, m=sp.num_voxels, min_rays=1), **bad))
    with pytest.raises(native.NativeError):
        native.accum_observed_lookup(pts, torch.zeros(4, 3, dtype=torch.int32, device=DEV), None, 0.1, sp._cur, sp.num_voxels, 1)


@pytest.mark.gpu
def test_gone_or_never_looked_at_gpu(host_exe, tmp_path):
    """The capability, C13's gap.  Session A's cloud holds the wall and the clusters K and U; session B scans only the wall.  A.difference(B) is K and U,
    54 voxels; B's observed space says which of them B's rays went through -- K, at least 4 rays each -- and which B never looked at -- U."""
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    space, _ = _capability()
    a = _session_a()
    b = AccumulatedCloud(0.1, DEV, 64)
    b.add(_t(WALL_CALL['points']), stamp=1)
    space_b = _observe(_space(0.1, 64), WALL_CALL, stamp=1)
    keys, rays, stamps = space_b.records()
    assert oref.table_of(keys, rays, stamps) == {c: [r[0], 1, 1] for c, r in space.rec.items()}
    assert space_b.counters == dict(zip(('walked', 'dropped', 'skipped', 'truncated', 'visits'), space.counters))
    gone = a.difference(b)
    coords = gone.extract()['coords']
    assert sorted(map(tuple, coords.tolist())) == sorted(CLUSTER_K + CLUSTER_U)
    seen = space_b.lookup_voxels(coords, min_rays=4)
    really_gone = (seen['status'] & native.OBSERVED_ENOUGH) != 0
    assert sorted(map(tuple, coords[really_gone].tolist())) == sorted(CLUSTER_K) and int(really_gone.sum()) == 27
    assert not bool((seen['status'][~really_gone] & native.OBSERVED_SEEN).any()) and seen['counters'].tolist() == [54, 54, 27, 27]
    assert bool((seen['rays'][really_gone] >= 4).all()) and int(space_b.lookup_voxels(coords, min_rays=5)['counters'][3]) < 27
    for rows, state in ((CLUSTER_K, oref.FREE), (CLUSTER_U, oref.UNKNOWN), (WALL, oref.OCCUPIED)):
        assert set(space_b.occupancy(b, _t(np.array(rows, np.int32))).tolist()) == {state}


@pytest.mark.gpu
def test_observe_results_on_the_model_forward_gpu(golden):
    """observe_results on the model_tiny_test forward: walked + dropped + skipped = n, and the result equals a direct observe with hand-built origins.
    Nothing more is claimed: its frames are independent random clouds."""
    from helpers import make_batch
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
    a = _space(0.2, 64).observe_results(out, inp, sensor_offset=offset, stamp=1, max_range=6.0)
    ego = out['ego_motion_est'][0].cpu().numpy().astype(np.float64)
    origins = ((ego[:, :3, 0] * offset[0] + ego[:, :3, 1] * offset[1]) + ego[:, :3, 2] * offset[2]) + ego[:, :3, 3]
    b = _space(0.2, 64).observe(out['rec_est'], origins, inp['time_indice'][:, 1], None, out['mos_est'].argmax(1) == 1, stamp=1, max_range=6.0)
    _assert_spaces_equal(a, b, 'results')
    c = a.counters
    assert c['walked'] + c['dropped'] + c['skipped'] == n and c['walked'] > 0 and int(a.extract()['rays'].sum()) == c['visits'] > 0
    with pytest.raises(ValueError):
        a.observe_results(dict(out, _n_batches=2), inp)
