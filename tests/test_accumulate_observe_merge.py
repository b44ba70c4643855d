"""Observed space, merged and re-voxelised (include/pcacc.h C15): ObservedSpace.copy / regrid / merge.

CPU leg: csrc/accum_observe_merge.h -- the code the kernels run -- built with g++ (-ffp-contract=off, every index assert-checked, poison behind the last
row, every destination written once) against the plain-Python restatement tests/accumulate_observe_merge_reference.py (dicts of coordinates, no keys, no
sort): every column, counter and state word EQUAL; the figures of the scenes checked on the restatement alone.
GPU leg: the kernels against the host build, integer for integer, on every case of the CPU leg; the set property; growth; the refusals by snapshot;
merge under a pose; copy; the argument checks; the capability -- a session in its own frame brought over, what is gone against what was never looked at;
occupancy after both merges.
Every result is an integer and the float64 pose path is held bit for bit: no test has a tolerance."""
import os

import numpy as np
import pytest
import torch

import accumulate_helpers as ah
import accumulate_observe_merge_reference as mref
import accumulate_observe_reference as oref
import test_accumulate_observe as c14
from accumulate_helpers import DEV, EDGE
from helpers import ROOT

NAN = float('nan')
STATE_WORDS = 16
NUM_VOXELS, STATUS, NEEDED, WALKED = 0, 1, 2, 6
OK, TOO_SMALL, BAD_STATE = 0, 1, 2
POISON_I64, POISON_I32 = 0x5b5b5b5b5b5b5b5b, 0x5c5c5c5c
POISON_KEY = 0x5a5a5a5a5a5a5a5a
CELLS = ah.block(-4, 4)                                                          # 512 voxels around the origin
TURN = ah.rot_xyz(0.0, 0.0, np.pi / 6, (0.37, -0.21, 0.04))                      # 30 degrees about z and a translation


# ---- tables of the restatement ---------------------------------------------------------------------------------------------------------------------
def _rows(coords, seed, vs=0.1):
    """Random records on the given voxels: rays 1..9, stamps 0..15, random counters -> ReferenceSpace."""
    rs = np.random.RandomState(seed)
    sp = oref.ReferenceSpace(vs)
    for c in np.asarray(coords).reshape(-1, 3).tolist():
        t = int(rs.randint(0, 11))
        sp.rec[tuple(c)] = [int(rs.randint(1, 10)), t, t + int(rs.randint(0, 6))]
    sp.counters = [int(v) for v in rs.randint(0, 1000, 5)]
    return sp


def _some(m, seed):
    return CELLS[np.random.RandomState(seed).permutation(len(CELLS))[:m]]


_cache = {}


def _once(name, make):
    """A scene of the restatement, computed once and never modified."""
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _halves():
    """C14's 400 random rays dealt into two spaces at two stamps, and the one space that observed everything."""
    def make():
        call = c14.CALLS['random']
        deal = np.random.RandomState(17).permutation(400)
        parts = [dict(call, points=call['points'][p], origin_index=call['origin_index'][p], stamp=s) for p, s in ((deal[:230], 5), (deal[230:], 3))]
        whole = oref.ReferenceSpace(0.1)
        for part in parts:
            c14._restate(part, whole)
        return parts, [c14._restate(part) for part in parts], whole
    return _once('halves', make)


def _three_calls():
    """C14's three-call sequence: A saw the first call, B the second and the third; and the one space that observed all three."""
    def make():
        calls = c14._sequence()
        a, b, whole = c14._restate(calls[0]), oref.ReferenceSpace(0.1), oref.ReferenceSpace(0.1)
        for call in calls[1:]:
            c14._restate(call, b)
        for call in calls:
            c14._restate(call, whole)
        return a, b, whole
    return _once('three', make)


def _bound_table():
    """Rows at the index bound on every axis (C14's bound scene: 0.01 m, where the centre of voxel 2^20 - 1 still lies below 32768 m)."""
    return _once('bound', lambda: c14._restate(c14.CALLS['bound']))


def _merge_cases():
    """name -> () -> dict(a=, b= (None: B is A), and optionally out_capacity=, a_words=, b_words=)."""
    cases = {}
    for ma in (0, 1, 63, 64, 65, 257):
        for mb in (0, 1, 63, 64, 65, 257):
            cases['size_%d_%d' % (ma, mb)] = lambda ma=ma, mb=mb: dict(a=_rows(_some(ma, 100 + ma), ma), b=_rows(_some(mb, 200 + mb), 1000 + mb))
    low, high = CELLS[CELLS[:, 0] < 0], CELLS[CELLS[:, 0] >= 0]
    cases['below'] = lambda: dict(a=_rows(high[::3], 1), b=_rows(low[::2], 2))
    cases['above'] = lambda: dict(a=_rows(low[::3], 3), b=_rows(high[::2], 4))
    cases['interleaved'] = lambda: dict(a=_rows(CELLS[::2], 5), b=_rows(CELLS[::3], 6))
    cases['identical'] = lambda: dict(a=_rows(CELLS[::5], 7), b=_rows(CELLS[::5], 8))
    cases['disjoint'] = lambda: dict(a=_rows(CELLS[::2], 9), b=_rows(CELLS[1::2], 10))
    cases['same'] = lambda: dict(a=_rows(CELLS[::3], 11), b=None)
    cases['halves'] = lambda: dict(a=_halves()[1][0], b=_halves()[1][1])
    cases['halves_swapped'] = lambda: dict(a=_halves()[1][1], b=_halves()[1][0])
    cases['three_calls'] = lambda: dict(a=_three_calls()[0], b=_three_calls()[1])
    return cases


MERGE_CASES = _merge_cases()


def _regrid_cases():
    """name -> () -> dict(space=, pose=, voxel_size=)."""
    random = lambda: c14._restated_call('random')
    cases = {'identity': lambda: dict(space=random(), pose=None, voxel_size=0.1),
             'identity_eye': lambda: dict(space=random(), pose=np.eye(4), voxel_size=None),
             'identity_bound': lambda: dict(space=_bound_table(), pose=np.eye(4), voxel_size=0.01),
             'shift': lambda: dict(space=random(), pose=ah.rot_xyz(0, 0, 0, (0.3, -0.2, 0.1)), voxel_size=None),
             'turn': lambda: dict(space=random(), pose=TURN, voxel_size=None),
             'turn_twice': lambda: dict(space=random(), pose=TURN, voxel_size=0.2),
             'push_up': lambda: dict(space=_bound_table(), pose=ah.rot_xyz(0, 0, 0, (0.01, 0.01, 0.01)), voxel_size=None),
             'push_down': lambda: dict(space=_bound_table(), pose=ah.rot_xyz(0, 0, 0, (-0.01, -0.01, -0.01)), voxel_size=None),
             'nan_pose': lambda: dict(space=_rows(CELLS[::7], 12), pose=np.full((4, 4), NAN), voxel_size=None)}
    for f in (2, 3, 5):
        cases['coarse%d' % f] = lambda f=f: dict(space=random(), pose=None, voxel_size=f * 0.1)
        cases['coarse%d_eye' % f] = lambda f=f: dict(space=random(), pose=np.eye(4), voxel_size=f * 0.1)
    for m in (0, 1, 64, 65):
        cases['rows%d' % m] = lambda m=m: dict(space=_rows(_some(m, 300 + m), 13 + m), pose=TURN, voxel_size=0.2)
    return cases


REGRID_CASES = _regrid_cases()


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------------
host_exe = ah.host_driver_fixture('accum_observe_merge_host_driver', 'accom')
SPARE = 3                                                                        # rows of capacity behind the rows in use


def _state_of(space, words=None):
    """The sixteen state words of a table: its rows and counters; words 1 - 5 and 11 - 15 hold values a call must zero or leave."""
    st = np.array([len(space.rec), 1, 99, 5, 7, 9] + list(space.counters) + [111, 112, 113, 114, 115], np.int64)
    for k, v in (words or {}).items():
        st[k] = v
    return st


def _merge_args(case):
    """-> (A's columns, A's state, B's columns or None, B's state or None, out_capacity)."""
    a, b = case['a'], case['b']
    want = mref.merge(a, a if b is None else b)[1]['rows']
    return (mref.columns(a), _state_of(a, case.get('a_words')), None if b is None else mref.columns(b), None if b is None else _state_of(b, case.get('b_words')),
            case.get('out_capacity', want + SPARE))


_host_cache = {}


def _host_merge(exe, tmp_path, tag, case):
    """The g++ build on one merge -> dict(counters [4], state [16], keys, rays, stamps: the rows written)."""
    if tag in _host_cache:
        return _host_cache[tag]
    at, ast, bt, bst, out_cap = _merge_args(case)
    ma, mb = at[0].shape[0], (at if bt is None else bt)[0].shape[0]
    chunks = [np.array([0, ma, ma + SPARE, mb, mb + SPARE, out_cap, bt is None, 0], np.int64)] + list(at) + [ast]
    if bt is not None:
        chunks += list(bt) + [bst]
    raw = ah.run_driver(exe, tmp_path, tag, *chunks, suffix='.bin')
    out, off = ah.unpack(raw, 0, [('counters', np.int64, (4,)), ('state', np.int64, (STATE_WORDS,)), ('rows', np.int64, (1,))])
    r = int(out['rows'][0])
    more, off = ah.unpack(raw, off, [('keys', np.int64, (r,)), ('rays', np.int64, (r,)), ('stamps', np.int32, (2, r))])
    assert off == len(raw)
    out.update(more)
    _host_cache[tag] = out
    return out


def _regrid_args(case):
    sp = case['space']
    return mref.columns(sp), _state_of(sp, case.get('words')), case['pose'], sp.voxel_size, sp.voxel_size if case['voxel_size'] is None else case['voxel_size']


def _host_regrid(exe, tmp_path, tag, case):
    """The g++ build on one regrid -> dict(counters [3], state [16], keys, rays, stamps)."""
    if tag in _host_cache:
        return _host_cache[tag]
    table, st, pose, in_vs, out_vs = _regrid_args(case)
    m = table[0].shape[0]
    raw = ah.run_driver(exe, tmp_path, tag, np.array([1, m, m + SPARE, m + SPARE, pose is not None, 0, 0, 0], np.int64), np.array([in_vs, out_vs], np.float64),
                        np.eye(4) if pose is None else np.ascontiguousarray(pose, np.float64), *table, st, suffix='.bin')
    out, off = ah.unpack(raw, 0, [('counters', np.int64, (3,)), ('state', np.int64, (STATE_WORDS,)), ('rows', np.int64, (1,))])
    r = int(out['rows'][0])
    more, off = ah.unpack(raw, off, [('keys', np.int64, (r,)), ('rays', np.int64, (r,)), ('stamps', np.int32, (2, r))])
    assert off == len(raw)
    out.update(more)
    _host_cache[tag] = out
    return out


def _merged_state(a_state, b_state, rows):
    want = a_state.copy()
    want[[NUM_VOXELS, STATUS, NEEDED, 3, 4, 5]] = [rows, OK, rows, 0, 0, 0]
    want[WALKED:WALKED + 5] += b_state[WALKED:WALKED + 5]
    return want


# ---- CPU: merge ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MERGE_CASES))
def test_merge_host_build_equals_the_restatement(host_exe, tmp_path, name):
    """Every column, the four counters and all sixteen state words: words 1 - 5 as the contract sets them, 11 - 15 untouched."""
    case = MERGE_CASES[name]()
    a, b = case['a'], case['a'] if case['b'] is None else case['b']
    want, info = mref.merge(a, b)
    h = _host_merge(host_exe, tmp_path, name, case)
    if not a.rec and not b.rec:                                                  # ma = mb = 0: the zero counters, and nothing else
        assert h['counters'].tolist() == [0, 0, 0, 0] and np.array_equal(h['state'], _state_of(a)) and h['keys'].shape[0] == 0
        return
    assert h['counters'].tolist() == [OK, info['rows'], info['shared'], info['new']], name
    assert oref.table_of(h['keys'], h['rays'], h['stamps']) == want.rec and h['keys'].shape[0] == len(want.rec), name
    assert np.all(h['keys'][1:] > h['keys'][:-1])
    assert np.array_equal(h['state'], _merged_state(_state_of(a), _state_of(b), len(want.rec))), name
    assert h['state'][WALKED:WALKED + 5].tolist() == want.counters


def test_merge_is_one_table_that_observed_everything():
    """The claim, on the restatement alone: the union of two sessions' tables and counters is the table of one session given every observe of both."""
    parts, (a, b), whole = _halves()
    for x, y in ((a, b), (b, a)):
        got, info = mref.merge(x, y)
        assert got.rec == whole.rec and got.counters == whole.counters
    assert len(whole.rec) == 6762 and whole.counters[oref.VISITS] == 10907 and info == dict(rows=6762, shared=len(a.rec) + len(b.rec) - 6762, new=6762 - len(b.rec))
    assert {(r[1], r[2]) for r in whole.rec.values()} == {(3, 3), (3, 5), (5, 5)}
    a, b, whole = _three_calls()
    got, info = mref.merge(a, b)
    assert got.rec == whole.rec and got.counters == whole.counters and info['shared'] > 1000 and info['new'] > 100
    twice, info = mref.merge(a, a)
    assert twice.rec == {c: [2 * r[0], r[1], r[2]] for c, r in a.rec.items()} and twice.counters == [2 * v for v in a.counters]
    assert info == dict(rows=len(a.rec), shared=len(a.rec), new=0)


def test_merge_refusals_in_the_host_build(host_exe, tmp_path):
    """TOO_SMALL one row below NEEDED leaves the poisoned outputs and the state (the driver asserts both) and says what it takes; exactly NEEDED goes
    through; BAD_STATE for either table addresses nothing."""
    base = MERGE_CASES['interleaved']()
    need = mref.merge(base['a'], base['b'])[1]['rows']
    h = _host_merge(host_exe, tmp_path, 'small', dict(base, out_capacity=need - 1))
    assert h['counters'].tolist()[:2] == [TOO_SMALL, need] and h['keys'].shape[0] == 0 and np.array_equal(h['state'], _state_of(base['a']))
    h = _host_merge(host_exe, tmp_path, 'exact', dict(base, out_capacity=need))
    assert h['counters'].tolist()[:2] == [OK, need] and h['keys'].shape[0] == need
    for tag, words in (('bad_a', dict(a_words={NUM_VOXELS: len(base['a'].rec) + 1})), ('bad_b', dict(b_words={NUM_VOXELS: len(base['b'].rec) - 1}))):
        h = _host_merge(host_exe, tmp_path, tag, dict(base, **words))
        assert h['counters'].tolist() == [BAD_STATE, 0, 0, 0] and h['keys'].shape[0] == 0
        assert np.array_equal(h['state'], _state_of(base['a'], words.get('a_words')))


REFUSALS = {'small': lambda: dict(MERGE_CASES['interleaved'](), out_capacity=mref.merge(MERGE_CASES['interleaved']()['a'], MERGE_CASES['interleaved']()['b'])[1]['rows'] - 1),
            'exact': lambda: dict(MERGE_CASES['interleaved'](), out_capacity=mref.merge(MERGE_CASES['interleaved']()['a'], MERGE_CASES['interleaved']()['b'])[1]['rows']),
            'bad_a': lambda: dict(MERGE_CASES['interleaved'](), a_words={NUM_VOXELS: len(MERGE_CASES['interleaved']()['a'].rec) + 1}),
            'bad_b': lambda: dict(MERGE_CASES['interleaved'](), b_words={NUM_VOXELS: len(MERGE_CASES['interleaved']()['b'].rec) - 1})}


# ---- CPU: regrid ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(REGRID_CASES))
def test_regrid_host_build_equals_the_restatement(host_exe, tmp_path, name):
    """Every column, the three counters and all sixteen words of the new state."""
    case = REGRID_CASES[name]()
    sp = case['space']
    want, dropped = mref.regrid(sp, case['pose'], case['voxel_size'])
    h = _host_regrid(host_exe, tmp_path, name, case)
    assert h['counters'].tolist() == [len(sp.rec), len(want.rec), dropped], name
    assert oref.table_of(h['keys'], h['rays'], h['stamps']) == want.rec and h['keys'].shape[0] == len(want.rec), name
    assert np.all(h['keys'][1:] > h['keys'][:-1])
    assert h['state'].tolist() == [len(want.rec), 0, 0, 0, 0, 0] + sp.counters + [0] * 5, name


def test_regrid_properties_in_the_restatement():
    """(a) identity at the same size is the same table, at the index bound too; (b) an integer multiple of the voxel size is floor division per axis, with
    runs longer than a wave for f = 5; a whole-voxel translation shifts the keys and keeps the records; rows pushed off the grid are dropped and none is
    clamped; a pose of NaN drops every row."""
    sp = c14._restated_call('random')
    for pose in (None, np.eye(4)):
        got, dropped = mref.regrid(sp, pose, None if pose is not None else 0.1)
        assert got.rec == sp.rec and dropped == 0 and got.counters == sp.counters
    bound = _bound_table()
    got, dropped = mref.regrid(bound, np.eye(4), 0.01)
    assert got.rec == bound.rec and dropped == 0 and any(EDGE - 1 in c for c in bound.rec) and any(-EDGE in c for c in bound.rec)
    for f in (2, 3, 5):
        got, dropped = mref.regrid(sp, None, f * 0.1)
        want, sources = {}, {}
        for c, r in sp.rec.items():
            d = tuple(v // f for v in c)                                         # integer floor division
            have = want.get(d)
            want[d] = list(r) if have is None else [max(have[0], r[0]), min(have[1], r[1]), max(have[2], r[2])]
            sources[d] = sources.get(d, 0) + 1
        assert got.rec == want and dropped == 0, f
        assert any(min(c) < 0 for c in sp.rec) and (f != 5 or max(sources.values()) > 64)
    shift, dropped = mref.regrid(sp, ah.rot_xyz(0, 0, 0, (0.3, -0.2, 0.1)))
    assert shift.rec == {(c[0] + 3, c[1] - 2, c[2] + 1): r for c, r in sp.rec.items()} and dropped == 0
    up, dropped_up = mref.regrid(bound, ah.rot_xyz(0, 0, 0, (0.01, 0.01, 0.01)))
    down, dropped_down = mref.regrid(bound, ah.rot_xyz(0, 0, 0, (-0.01, -0.01, -0.01)))
    assert dropped_up == 3 == len([c for c in bound.rec if EDGE - 1 in c]) and dropped_down == 3 == len([c for c in bound.rec if -EDGE in c])
    assert up.rec == {tuple(v + 1 for v in c): r for c, r in bound.rec.items() if EDGE - 1 not in c}
    assert down.rec == {tuple(v - 1 for v in c): r for c, r in bound.rec.items() if -EDGE not in c}
    nothing, dropped = mref.regrid(_rows(CELLS[::7], 12), np.full((4, 4), NAN))
    assert nothing.rec == {} and dropped == len(CELLS[::7])
    turned, dropped = mref.regrid(sp, TURN)
    assert dropped == 0 and len(turned.rec) < len(sp.rec) and max(r[0] for r in turned.rec.values()) == 147     # lossy: centres share voxels


def test_regrid_bad_state_in_the_host_build(host_exe, tmp_path):
    """out_state[STATUS] is the only word written: the counters stay zero, the other fifteen words and the output table stay poison."""
    sp = _rows(_some(65, 1), 2)
    h = _host_regrid(host_exe, tmp_path, 'bad_state', dict(space=sp, pose=TURN, voxel_size=0.2, words={NUM_VOXELS: 64}))
    assert h['counters'].tolist() == [0, 0, 0] and h['keys'].shape[0] == 0
    assert h['state'].tolist() == [POISON_I64, BAD_STATE] + [POISON_I64] * 14


BAD_REGRID = lambda: dict(space=_rows(_some(65, 1), 2), pose=TURN, voxel_size=0.2, words={NUM_VOXELS: 64})


# ---- CPU: the capability scene -----------------------------------------------------------------------------------------------------------------------
SESSION_POSE = ah.rot_xyz(0.0, 0.0, np.pi / 6, (0.37, -0.21, 0.04))              # session B's frame to session A's


def _session_b():
    """Session B scans only the wall, in ITS OWN frame: the wall points and the sensor of C14's scene under the inverse of SESSION_POSE.
    -> (the call, B's space on the restatement)."""
    def make():
        inv = np.linalg.inv(SESSION_POSE)
        pts = (c14.WALL_CALL['points'].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        org = ah.GHOST_SENSOR @ inv[:3, :3].T + inv[:3, 3]
        call = dict(vs=0.1, points=pts, origins=org, margin=0.2, stamp=1)
        return call, c14._restate(call)
    return _once('session_b', make)


def _coarse(rows):
    return [tuple(v // 2 for v in c) for c in rows]


def test_capability_scene_in_the_restatement():
    """B's table brought into A's frame at twice the voxel size: every voxel of K lies in a seen coarse voxel, none of U does.  At the SAME voxel size the
    rotated centres leave holes: K is not wholly seen, which is why regrid's docstring asks for a coarser size with a rotation."""
    _, space_b = _session_b()
    assert space_b.counters[:4] == [800, 0, 0, 0] and len(space_b.rec) == 7655
    moved, dropped = mref.regrid(space_b, SESSION_POSE, 0.2)
    assert dropped == 0 and len(moved.rec) == 1206
    assert all(c in moved.rec for c in _coarse(c14.CLUSTER_K)) and not any(c in moved.rec for c in _coarse(c14.CLUSTER_U))
    assert min(moved.rec[c][0] for c in _coarse(c14.CLUSTER_K)) == 6
    same, _ = mref.regrid(space_b, SESSION_POSE, 0.1)
    assert len([c for c in c14.CLUSTER_K if c in same.rec]) == 21 and not any(c in same.rec for c in c14.CLUSTER_U)


def test_header_binding_and_argument_checks():
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud, ObservedSpace
    header = open(os.path.join(ROOT, 'include', 'pcacc.h')).read()
    for name in ('pcacc_accum_observed_merge_workspace_bytes', 'pcacc_accum_observed_merge', 'pcacc_accum_observed_regrid_workspace_bytes',
                 'pcacc_accum_observed_regrid'):
        assert ('int %s(' % name) in header and name in native.EXPORTS
    assert ' C15. ' in header
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'csrc', 'accum_observe_merge.h')).read()
    assert [l for l in text.split('\n') if l.startswith('#include')] == ['#include "accum_observe.h"', '#include "accum_merge.h"']
    assert text.count('PCACC_BOUND(') >= 10
    a, b = ObservedSpace(0.1, 'cpu', 64), ObservedSpace(0.2, 'cpu', 64)
    with pytest.raises(TypeError):
        a.merge(AccumulatedCloud(0.1, 'cpu', 64))
    with pytest.raises(ValueError, match='voxel sizes'):
        a.merge(b)
    with pytest.raises(ValueError, match='regrid needs'):
        a.regrid()
    for bad in (dict(voxel_size=0.0), dict(voxel_size=NAN), dict(voxel_size=0.2, capacity=0), dict(pose=np.eye(3))):
        with pytest.raises(ValueError):
            a.regrid(**bad)
    with pytest.raises(ValueError):
        a.merge(b, pose=np.eye(3))
    for call in (lambda: a.regrid(voxel_size=0.2), lambda: a.merge(ObservedSpace(0.1, 'cpu', 64)), lambda: a.merge(b, pose=np.eye(4))):
        with pytest.raises(native.NativeError):
            call()
    c = a.copy()
    assert (c.voxel_size, c.capacity, c.visit_budget, c.num_voxels, c.counters, c.splits, c.dropped_rows) == (0.1, 64, a.visit_budget, 0, a.counters, 0, 0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------
def _t(v, dtype=None):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype)).to(DEV)


def _device_table(columns, capacity, fills=(0, 77, -7)):
    """The columns at the head of tables of `capacity` rows; behind them what the host driver puts there."""
    keys, rays, stamps = columns
    m = keys.shape[0]
    room = max(capacity, 1)
    out = (torch.full((room,), fills[0], dtype=torch.int64, device=DEV), torch.full((room,), fills[1], dtype=torch.int64, device=DEV),
           torch.full((2, room), fills[2], dtype=torch.int32, device=DEV))
    out[0][:m], out[1][:m], out[2][:, :m] = _t(keys), _t(rays), _t(stamps)
    return out


def _poison(capacity):
    room = max(capacity, 1)
    return (torch.full((room,), POISON_KEY, dtype=torch.int64, device=DEV), torch.full((room,), POISON_I64, dtype=torch.int64, device=DEV),
            torch.full((2, room), POISON_I32, dtype=torch.int32, device=DEV))


def _assert_out_is_host(out, h, what):
    """The rows the host build wrote, and poison behind them."""
    rows = h['keys'].shape[0]
    for t, f in zip(out, ('keys', 'rays', 'stamps')):
        assert torch.equal(t[..., :rows].cpu(), torch.from_numpy(h[f])), (what, f)
    assert bool((out[0][rows:] == POISON_KEY).all()) and bool((out[1][rows:] == POISON_I64).all()) and bool((out[2][:, rows:] == POISON_I32).all()), what


def _gpu_merge(case, h, what):
    from pcaccumulation_amd import native
    at, ast, bt, bst, out_cap = _merge_args(case)
    ma = at[0].shape[0]
    a = _device_table(at, ma + SPARE)
    state = _t(ast)
    b, b_state = (a, state) if bt is None else (_device_table(bt, bt[0].shape[0] + SPARE), _t(bst))
    mb = ma if bt is None else bt[0].shape[0]
    out = _poison(out_cap)
    counters = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    snap = [t.clone() for t in a + b] + [b_state.clone()]
    native.accum_observed_merge(a, ma, b, mb, b_state, out, counters, state)
    assert counters.tolist() == h['counters'].tolist() and state.tolist() == h['state'].tolist(), what
    _assert_out_is_host(out, h, what)
    for got, want in zip(list(a + b) + ([b_state] if bt is not None else []), snap):      # the inputs are as they were
        assert torch.equal(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(MERGE_CASES) + sorted(REFUSALS))
def test_merge_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """The same header, integers only: the counters, the sixteen state words, every row written and the poison behind them; the inputs untouched.  The
    refusals by snapshot: TOO_SMALL and BAD_STATE leave the poisoned outputs and the state as they were."""
    case = (MERGE_CASES.get(name) or REFUSALS[name])()
    h = _host_merge(host_exe, tmp_path, name, case)
    if name in ('small', 'bad_a', 'bad_b'):
        assert h['counters'][0] != OK and h['keys'].shape[0] == 0 and np.array_equal(h['state'], _state_of(case['a'], case.get('a_words')))
    _gpu_merge(case, h, name)


def _gpu_regrid(case, h, what):
    from pcaccumulation_amd import native
    table, st, pose, in_vs, out_vs = _regrid_args(case)
    m = table[0].shape[0]
    src = _device_table(table, m + SPARE)
    in_state = _t(st)
    out = _poison(m + SPARE)
    counters = torch.full((3,), -5, dtype=torch.int64, device=DEV)
    out_state = torch.full((STATE_WORDS,), POISON_I64, dtype=torch.int64, device=DEV)
    snap = [t.clone() for t in src] + [in_state.clone()]
    native.accum_observed_regrid(src, m, in_state, _t(pose, np.float64), in_vs, out_vs, out, counters, out_state)
    assert counters.tolist() == h['counters'].tolist() and out_state.tolist() == h['state'].tolist(), what
    _assert_out_is_host(out, h, what)
    for got, want in zip(list(src) + [in_state], snap):
        assert torch.equal(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(REGRID_CASES) + ['bad_state'])
def test_regrid_kernel_equals_the_host_build_gpu(host_exe, tmp_path, name):
    """The float64 pose path bit for bit, the fold by integer atomics: every column, counter and state word, the poison behind the last row."""
    case = BAD_REGRID() if name == 'bad_state' else REGRID_CASES[name]()
    _gpu_regrid(case, _host_regrid(host_exe, tmp_path, name, case), name)


def _space(vs=0.1, capacity=1 << 14):
    return c14._space(vs, capacity)


def _assert_space_is(sp, want, what):
    """A device space against a table of the restatement: the columns, the counters, the state words."""
    keys, rays, stamps = sp.records()
    assert oref.table_of(keys, rays, stamps) == want.rec and sp.num_voxels == len(want.rec) and np.all(keys[1:] > keys[:-1]), what
    assert list(sp.counters.values()) == want.counters, what
    state = sp._state.tolist()
    assert state[NUM_VOXELS] == sp.num_voxels and state[WALKED:WALKED + 5] == want.counters, what


@pytest.mark.gpu
def test_set_property_gpu():
    """The random rays dealt into two spaces at two stamps: A.merge(B) and B.merge(A) equal, in all four columns and the five counters, one space that
    observed everything; A.copy().merge(A) doubles every ray count and the counters and nothing else."""
    parts, (ra, rb), whole = _halves()
    one = _space()
    for part in parts:
        c14._observe(one, part)
    a, b = c14._observe(_space(), parts[0]), c14._observe(_space(), parts[1])
    snap_b = [c.clone() for c in c14._columns(b)] + [b._state.clone()]
    ab = a.copy()
    info = ab.merge(b)
    c14._assert_spaces_equal(ab, one, 'A.merge(B)')
    assert info == dict(mref.merge(ra, rb)[1], dropped_rows=0) and torch.equal(ab._state[[NUM_VOXELS, STATUS, NEEDED]].cpu(), torch.tensor([6762, 0, 6762]))
    for got, want in zip(c14._columns(b) + [b._state], snap_b):                 # `other` is never modified
        assert torch.equal(got, want)
    ba = b.copy()
    ba.merge(a)
    c14._assert_spaces_equal(ba, one, 'B.merge(A)')
    _assert_space_is(ab, whole, 'restatement')
    twice = a.copy()
    info = twice.merge(a)
    assert info == dict(rows=a.num_voxels, shared=a.num_voxels, new=0, dropped_rows=0)
    _assert_space_is(twice, mref.merge(ra, ra)[0], 'twice')
    keys, rays, t0, t1 = c14._columns(a)
    assert [torch.equal(x, y) for x, y in zip(c14._columns(twice), (keys, 2 * rays, t0, t1))] == [True] * 4
    self_merge = a.copy()
    self_merge.merge(self_merge)                                                 # A == B: the same tables and state words
    c14._assert_spaces_equal(self_merge, twice, 'self')
    empty = _space()
    before = c14._columns(a)
    assert a.merge(empty) == dict(rows=a.num_voxels, shared=0, new=0, dropped_rows=0)     # an empty `other` changes nothing
    assert all(torch.equal(x, y) for x, y in zip(c14._columns(a), before))
    into_empty = _space(0.1, 64)
    into_empty.merge(b)
    c14._assert_spaces_equal(into_empty, b, 'into an empty space')


@pytest.mark.gpu
def test_merge_grows_the_table_gpu():
    """A capacity of 64 growing through the merge of C14's wall scene: one ray in A, the other 799 in B, and the result is the table of all 800."""
    call = c14.WALL_CALL
    a = c14._observe(_space(0.1, 64), call, points=call['points'][:1])
    b = c14._observe(_space(0.1, 64), call, points=call['points'][1:])
    wall = c14._observe(_space(), call)
    assert a.capacity == 64
    info = a.merge(b)
    assert a.capacity == 8192 and a._cur[0].shape[0] == 8192 and info['rows'] == 7518 == info['shared'] + info['new'] + (7518 - b.num_voxels)
    c14._assert_spaces_equal(a, wall, 'grown')
    c14._observe(a, call, stamp=2)                                               # the table goes on from the merge
    assert a.num_voxels == 7518 and a.counters['walked'] == 1600


@pytest.mark.gpu
def test_merge_under_a_pose_and_regrid_gpu():
    """merge(other, pose) equals regrid then merge of the restatement; regrid returns a new space with the rows dropped as an attribute and leaves this one;
    coarsening by voxel_size alone."""
    parts, (ra, rb), _ = _halves()
    a, b = c14._observe(_space(), parts[0]), c14._observe(_space(0.1, 64), parts[1])
    snap_b = [c.clone() for c in c14._columns(b)]
    moved, dropped = mref.regrid(rb, TURN, 0.1)
    want, info = mref.merge(ra, moved)
    got = a.copy()
    assert got.merge(b, pose=TURN) == dict(info, dropped_rows=dropped)
    _assert_space_is(got, want, 'merge under a pose')
    assert all(torch.equal(x, y) for x, y in zip(c14._columns(b), snap_b))
    coarse = _space(0.2)
    coarse.merge(b, pose=np.eye(4))                                              # a finer table into a coarser one
    _assert_space_is(coarse, mref.regrid(rb, np.eye(4), 0.2)[0], 'coarser')
    r = b.regrid(voxel_size=0.5)
    assert r is not b and r.voxel_size == 0.5 and r.capacity == b.capacity and r.dropped_rows == 0 and r.visit_budget == b.visit_budget
    _assert_space_is(r, mref.regrid(rb, None, 0.5)[0], 'regrid')
    bound = c14._observe(_space(0.01, 64), c14.CALLS['bound'])
    pushed = bound.regrid(pose=ah.rot_xyz(0, 0, 0, (0.01, 0.01, 0.01)), capacity=32)
    assert pushed.dropped_rows == 3 and pushed.capacity == 32
    _assert_space_is(pushed, mref.regrid(_bound_table(), ah.rot_xyz(0, 0, 0, (0.01, 0.01, 0.01)))[0], 'pushed')
    seen = pushed.lookup_voxels(_t(np.array([[EDGE - 1, 1, -2], [EDGE - 2, 2, -1]], np.int32)))['status'].tolist()
    assert seen == [1, 7]                                                        # nothing was clamped onto the last voxel
    with pytest.raises(ValueError, match='capacity'):
        bound.regrid(voxel_size=0.02, capacity=bound.num_voxels - 1)


@pytest.mark.gpu
def test_copy_is_independent_gpu():
    """Observing into the copy leaves the original's tables and state, and the reverse."""
    parts, _, _ = _halves()
    a = c14._observe(_space(0.1, 8192), parts[0])
    snap = [c.clone() for c in c14._columns(a)] + [a._state.clone()]
    c = a.copy()
    c14._assert_spaces_equal(c, a, 'copy')
    assert torch.equal(c._state, a._state) and c._cur[0].data_ptr() != a._cur[0].data_ptr() and c._state.data_ptr() != a._state.data_ptr()
    assert (c.capacity, c.visit_budget, c.splits) == (a.capacity, a.visit_budget, 0)
    c14._observe(c, parts[1])
    for got, want in zip(c14._columns(a) + [a._state], snap):
        assert torch.equal(got, want)
    c14._observe(a, parts[1])
    c14._assert_spaces_equal(c, a, 'both went on alike')
    assert _space().copy().num_voxels == 0


@pytest.mark.gpu
def test_argument_checks_gpu():
    """Bad arguments raise before anything is allocated; the entry points answer PCACC_E_ARG and leave the state."""
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud, ObservedSpace
    a, b = _space(0.1, 64), _space(0.2, 64)
    for call, error in ((lambda: a.merge(AccumulatedCloud(0.1, DEV, 64)), TypeError), (lambda: a.merge(None), TypeError), (lambda: a.merge(b), ValueError),
                        (lambda: a.merge(ObservedSpace(0.1, 'cpu', 64)), ValueError), (lambda: a.merge(b, pose=np.eye(3)), ValueError),
                        (lambda: a.regrid(), ValueError), (lambda: a.regrid(voxel_size=-1.0), ValueError), (lambda: a.regrid(pose=np.zeros((3, 4))), ValueError),
                        (lambda: a.regrid(voxel_size=0.2, capacity=1 << 31), ValueError)):
        with pytest.raises(error):
            call()
    assert a._cur is None and a._state is None and b._cur is None
    sp = c14._observe(_space(0.25, 64), c14.CALLS['ties'])
    m, out = sp.num_voxels, tuple(torch.empty_like(t) for t in sp._cur)
    counters, counters3 = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    state = sp._state.clone()
    good = dict(tables_a=sp._cur, ma=m, tables_b=sp._cur, mb=m, b_state=sp._state, tables_out=out, counters=counters, state=sp._state)
    for bad in (dict(ma=65), dict(ma=-1), dict(mb=65), dict(mb=-1), dict(tables_out=sp._cur), dict(tables_out=(out[0], sp._cur[1], out[2]))):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_observed_merge(**dict(good, **bad))
    good_r = dict(tables_in=sp._cur, m=m, in_state=sp._state, pose=None, in_voxel_size=0.25, out_voxel_size=0.5, tables_out=out, counters=counters3,
                  out_state=torch.zeros(16, dtype=torch.int64, device=DEV))
    small = tuple(t[..., :m - 1].contiguous() for t in out)
    for bad in (dict(m=65), dict(m=-1), dict(in_voxel_size=0.0), dict(in_voxel_size=NAN), dict(out_voxel_size=0.0), dict(out_voxel_size=float('inf')),
                dict(tables_out=sp._cur), dict(tables_out=small)):
        with pytest.raises(native.NativeError, match='PCACC_E_ARG'):
            native.accum_observed_regrid(**dict(good_r, **bad))
    assert torch.equal(sp._state, state)
    native.accum_observed_regrid(**good_r)
    assert counters3.tolist() == [m, 4, 0]                                       # the ten voxels of `ties` on a grid of twice the size: a diagonal of four


def _session_a():
    return c14._session_a()


@pytest.mark.gpu
def test_session_in_its_own_frame_gpu():
    """The capability.  Session A's cloud holds the wall and the clusters K and U.  Session B scans only the wall in ITS OWN frame, a 30 degree turn about z
    and a translation away from A's.  B's cloud and B's observed space are brought into A's frame; A.difference(B) is K and U, and B's space -- at twice
    the voxel size, as regrid's docstring advises with a rotation -- marks every voxel of K seen and every voxel of U never looked at."""
    from pcaccumulation_amd import native
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    call, space_b = _session_b()
    a = _session_a()
    b_cloud = AccumulatedCloud(0.1, DEV, 64)
    b_cloud.add(_t(call['points']), stamp=1)
    b_space = c14._observe(_space(0.1, 64), call)
    _assert_space_is(b_space, space_b, 'session B')
    moved = b_space.regrid(SESSION_POSE, 0.2)
    assert moved.dropped_rows == 0 and moved.voxel_size == 0.2 and b_space.num_voxels == 7655
    _assert_space_is(moved, mref.regrid(space_b, SESSION_POSE, 0.2)[0], 'moved')
    gone = a.difference(b_cloud.regrid(SESSION_POSE))
    coords = gone.extract()['coords']
    assert sorted(map(tuple, coords.tolist())) == sorted(c14.CLUSTER_K + c14.CLUSTER_U)
    seen = moved.lookup_voxels(torch.div(coords, 2, rounding_mode='floor'), min_rays=6)
    really_gone = (seen['status'] & native.OBSERVED_ENOUGH) != 0
    assert sorted(map(tuple, coords[really_gone].tolist())) == sorted(c14.CLUSTER_K) and int(really_gone.sum()) == 27
    assert not bool((seen['status'][~really_gone] & native.OBSERVED_SEEN).any()) and seen['counters'].tolist() == [54, 54, 27, 27]
    assert int(moved.lookup_voxels(torch.div(coords, 2, rounding_mode='floor'), min_rays=7)['counters'][3]) < 27


@pytest.mark.gpu
def test_occupancy_after_both_merges_gpu():
    """Two sessions on one grid: merge the clouds, merge the spaces, occupancy still answers -- and equals the restatement's on the merged table."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    wall_space, _ = c14._capability()
    sensor2 = np.array([[0.03, 1.42, 0.01]])                                     # session B looks at the wall from beside cluster U
    call_b = dict(c14.WALL_CALL, origins=sensor2, stamp=1)
    space_b = c14._restate(call_b)
    want, _ = mref.merge(wall_space, space_b)
    cloud_a = _session_a()
    cloud_b = AccumulatedCloud(0.1, DEV, 64)
    cloud_b.add(_t(c14.WALL_CALL['points']), stamp=1)
    sp = c14._observe(_space(0.1, 64), c14.WALL_CALL)
    sp.merge(c14._observe(_space(0.1, 64), call_b))
    cloud_a.merge(cloud_b)
    _assert_space_is(sp, want, 'merged')
    rows = c14.WALL[::7] + c14.CLUSTER_K + c14.CLUSTER_U + [(0, 0, 0), (0, 14, 0), (5, 1, 0), (5, 12, 0), (40, 0, 0), (EDGE - 1, 0, 0)]
    coords = np.array(rows + [(EDGE, 0, 0)], np.int64)
    occupied = set(c14.WALL + c14.CLUSTER_K + c14.CLUSTER_U)
    states = {}
    for min_rays in (1, 5, 801):
        got = sp.occupancy(cloud_a, _t(coords), min_rays=min_rays)
        assert got.tolist() == want.occupancy(occupied, coords, min_rays), min_rays
        states[min_rays] = got.tolist()
    assert set(states[1]) == {oref.UNKNOWN, oref.FREE, oref.OCCUPIED} and states[1][-7:] == [oref.FREE] * 4 + [oref.UNKNOWN] * 3
    assert states[801][-7:] == [oref.UNKNOWN] * 7                                # both sensors' own voxels: 800 rays each
    assert want.occupancy(set(), [(5, 12, 0)], 1) == [oref.FREE] and wall_space.occupancy(set(), [(5, 12, 0)], 1) == [oref.UNKNOWN]     # only B looked there
