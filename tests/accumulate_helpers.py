"""What the tests of the accumulated scene cloud share (tests/test_accumulate*.py): the scene builders, the files of the host
drivers (tests/accum_host.h), the way from a restatement's map to a device map, and the snapshot that says "this call left the map unchanged".

Every builder is a pure function of its arguments and returns fresh arrays.  torch and pcaccumulation_amd are imported where they are needed: the
module loads, and every CPU test runs, without the native library."""
import io
import os
import subprocess

import numpy as np

import accumulate_merge_reference as mref
import accumulate_prune_reference as rref
import accumulate_reference as ref

DEV = 'cuda:0'
EDGE = 1 << 20                                                                   # voxel indices lie in [-EDGE, EDGE)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
CORNER = np.array([0.43, -1.21, 0.27])                                           # where the three sheets of the room corner meet (section 9e)
GHOST_SENSOR = np.array([[0.03, 0.02, 0.01]])                                    # the fixed sensor of the ghost scene (section 9f)


# ---- poses and points -------------------------------------------------------------------------------------------------------------------------------
def rot_axis(axis, angle, t):
    """Rodrigues: a rotation by `angle` about `axis` and a translation, [4,4] f64."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def rot_xyz(rx, ry, rz, t):
    """Rotations about x, y, z (radians, composed z y x) and a translation, [4,4] f64."""
    T = np.eye(4)
    for axis, a in ((0, rx), (1, ry), (2, rz)):
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        R = np.eye(4)
        R[i, i], R[i, j], R[j, i], R[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        T = R @ T
    T[:3, 3] = t
    return T


def centres(idx, vs):
    """The centres of the voxels `idx` [..,3] -> [N,3] f32."""
    return ((np.asarray(idx, np.float64).reshape(-1, 3) + 0.5) * vs).astype(np.float32)


def block(lo, hi):
    """Every voxel index of the cube [lo, hi)^3, x slowest -> [N,3] int."""
    g = np.arange(lo, hi)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def wavy(shift=0.0):
    """26 m x 26 m at 0.1 m, four points in every column, and one far voxel -- 76 661 voxels: more than one workgroup, m mod 64 != 0, more than one
    scan chunk (the sheet of section 9d); `shift` moves it along x."""
    g = np.arange(520) * 0.05 + 0.025 - 13.0
    x, y = np.meshgrid(g, g, indexing='ij')
    z = 0.4 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.013
    pts = np.concatenate([np.stack([x, y, z], -1).reshape(-1, 3), [[40.0, 40.0, 40.0]]])
    pts[:, 0] += shift
    return pts.astype(np.float32)


def noisy_plane():
    """A 3 m x 3 m sheet with 1 cm noise and forty single points scattered above it."""
    rs = np.random.RandomState(21)
    sheet = np.concatenate([rs.uniform(-1.5, 1.5, (6000, 2)), rs.normal(0.02, 0.01, (6000, 1))], 1)
    stray = np.concatenate([rs.uniform(-1.5, 1.5, (40, 2)), rs.uniform(0.4, 2.0, (40, 1))], 1)
    return np.concatenate([sheet, stray]).astype(np.float32)


def corner(seed, per_sheet, noise=0.01):
    """Three mutually orthogonal noisy sheets of 2 m x 2 m that meet in CORNER (world frame, float64)."""
    rs = np.random.RandomState(seed)
    sheets = []
    for axis in range(3):
        p = rs.uniform(0.0, 2.0, (per_sheet, 3))
        p[:, axis] = rs.normal(0, noise, per_sheet)
        sheets.append(p + CORNER)
    return np.concatenate(sheets)


def random_rays():
    """400 rays: origins within +-0.3 m (row 0 float32-representable, so that a component of d can be exactly zero), end points within +-2 m.
    -> points [400,3] f32, origins [3,3] f64, origin index [400] i32."""
    rs = np.random.RandomState(11)
    origins = rs.uniform(-0.3, 0.3, (3, 3))
    origins[0] = origins[0].astype(np.float32)
    index = rs.randint(0, 3, 400).astype(np.int32)
    pts = rs.uniform(-2, 2, (400, 3)).astype(np.float32)
    o0 = origins[0].astype(np.float32)
    index[:24] = 0
    pts[0:6, 0] = o0[0]                                                          # d_x == 0 exactly
    pts[6:10, 1] = o0[1]                                                         # d_y == 0
    pts[10:14, 2] = o0[2]                                                        # d_z == 0
    for j, (axis, sign) in enumerate([(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]):    # along one axis: two zero components
        pts[14 + j] = o0
        pts[14 + j, axis] += np.float32(sign * (1.1 + 0.1 * j))
    pts[20:22, 0], pts[20:22, 1] = o0[0], o0[1]
    return pts, origins, index


def ghost_scans():
    """Six scans from GHOST_SENSOR: a wall one voxel layer thick at x = 3.05 (end points mid-layer) and a 3 x 3 x 3 cluster of voxel centres, never
    flagged moving, at a different y in front of the wall at each stamp.  Wall returns whose ray would have crossed the cluster of their own stamp are
    left out (the cluster shadows them).  -> [(wall points, cluster points, cluster voxels)]."""
    vs = 0.1
    wall = centres([(30, y, z) for y in range(-20, 20) for z in range(-10, 10)], vs)
    scans = []
    for k in range(6):
        y0 = -8 + 3 * k
        vox = [(15 + a, y0 + b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
        s = GHOST_SENSOR[0]
        t = (1.55 - s[0]) / (wall[:, 0].astype(np.float64) - s[0])                # where the wall ray passes the cluster's depth
        y = s[1] + t * (wall[:, 1] - s[1])
        z = s[2] + t * (wall[:, 2] - s[2])
        shadow = (np.abs(y - (y0 + 0.5) * vs) < 0.3) & (np.abs(z - 0.05) < 0.3)
        scans.append((wall[~shadow], centres(vox, vs), vox))
    return scans


# ---- the index bound: voxels next to -2^20 and 2^20 - 1 ---------------------------------------------------------------------------------------------
def _decoys(vox):
    """Where a key with an overflowed y or z field would land had an offset or a walk stepped past the edge: (x, 2^20, z) aliases (x+1, -2^20, z),
    (x, y, 2^20) aliases (x, y+1, -2^20), and the mirror images."""
    decoys = []
    for x, y, z in vox:
        if y == EDGE - 1:
            decoys.append((x + 1, -EDGE, z))
        if y == -EDGE:
            decoys.append((x - 1, EDGE - 1, z))
        if z == EDGE - 1:
            decoys.append((x, y + 1, -EDGE))
        if z == -EDGE:
            decoys.append((x, y - 1, EDGE - 1))
    return decoys


def bound_voxels():
    """3 x 3 columns through the last three voxels of every axis at both ends (3 x 3 x 3 clusters that touch -2^20 and 2^20 - 1), and the decoys
    that lie inside the grid.  -> two lists of (x, y, z)."""
    vox = []
    for axis in range(3):
        for lo in (-EDGE, EDGE - 3):
            for a in range(3):
                for b in (-1, 0, 1):
                    for c in (-1, 0, 1):
                        v = [b, c]
                        v.insert(axis, lo + a)
                        vox.append(tuple(v))
    return vox, [d for d in _decoys(vox) if all(-EDGE <= c < EDGE for c in d)]


def walked_voxels():
    """The last three voxels of every axis at both ends, which the bound scene's rays walk, and their decoys.  -> two lists of (x, y, z)."""
    walked = []
    for axis in range(3):
        for lo in (-EDGE, EDGE - 3):
            for a in range(3):
                v = [1, -2]
                v.insert(axis, lo + a)
                walked.append(tuple(v))
    return walked, _decoys(walked)


# ---- restated maps ----------------------------------------------------------------------------------------------------------------------------------
key = rref.key_of                                                                # (x, y, z) -> the 63-bit key


def records(vs, rows):
    """rows: {coord: (count, moving[, t_first, t_last])} -> a ReferenceMap whose coordinate sums put every centroid in the middle of its voxel."""
    r = ref.ReferenceMap(vs)
    for c, row in rows.items():
        count, moving, t_first, t_last = (tuple(row) + (0, 0))[:4]
        q = [int(np.rint((v + 0.5) * vs * 65536.0)) for v in c]
        r.rec[key(c)] = [count, moving, count * q[0], count * q[1], count * q[2], t_first, t_last]
    return r


def points_map(vs, adds):
    """adds: [(points, moving or None, stamp)] -> the ReferenceMap after them."""
    r = ref.ReferenceMap(vs)
    for pts, mv, stamp in adds:
        r.add(pts, None, mv, stamp)
    return r


def random_rows(m, seed):
    """m voxels of the 7^3 block around the origin with random records, stamps 0..15 and ray counts 0..4 -> records()'s rows, {coord: rays}."""
    rs = np.random.RandomState(seed)
    cells = [(x, y, z) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)]
    rows, pierced = {}, {}
    for i in rs.permutation(len(cells))[:m]:
        count = int(rs.randint(1, 7))
        t_first = int(rs.randint(0, 11))
        rows[cells[i]] = (count, int(rs.randint(0, count + 1)), t_first, t_first + int(rs.randint(0, 6)))
        p = int(rs.randint(0, 5))
        if p:
            pierced[cells[i]] = p
    return rows, pierced


def aligned(pierced, keys):
    """The ray counts of a {coord: rays} dict as the int32 column beside `keys` (for a {key: rays} dict: accumulate_merge_reference.aligned)."""
    return np.array([pierced.get(rref.coord_of(int(k)), 0) for k in keys.tolist()], np.int32)


CELLS = [(x, y, z) for x in range(-2, 3) for y in range(-2, 3) for z in range(-2, 3)]


def some(m, seed):
    """m of the 5^3 CELLS around the origin."""
    return [CELLS[i] for i in np.random.RandomState(seed).permutation(len(CELLS))[:m]]


def rows(coords, seed, rays=False, vs=0.1):
    """Random records on the given voxels: counts 1..6, stamps 0..15, centroids inside the voxel; rays 0..4 with rays=True.
    -> (ReferenceMap, {key: rays} or None)."""
    rs = np.random.RandomState(seed)
    r, p = ref.ReferenceMap(vs), ({} if rays else None)
    for c in coords:
        count = int(rs.randint(1, 7))
        t_first = int(rs.randint(0, 11))
        q = [int(np.rint((v + rs.uniform(0.1, 0.9)) * vs * 65536.0)) * count + int(rs.randint(0, count)) for v in c]
        r.rec[key(c)] = [count, int(rs.randint(0, count + 1))] + q + [t_first, t_first + int(rs.randint(0, 6))]
        if rays:
            p[key(c)] = int(rs.randint(0, 5))
    r.dropped = int(rs.randint(0, 9))
    return r, p


def window(k):
    """2049 random points in a 6 m x 6 m x 3 m box with flags, a stamp and a pose; two of them not finite."""
    rs = np.random.RandomState(70 + k)
    pts = rs.uniform((-3, -3, -1.5), (3, 3, 1.5), (2049, 3)).astype(np.float32)
    pts[5 + k] = np.nan
    pts[900 + 7 * k, 1] = np.inf
    return pts, rs.uniform(0, 1, 2049) < 0.3, 10 - 3 * k if k % 2 else k, rot_axis((0.1 * k, 1.0, 0.3), 0.02 * k, (0.05 * k, -0.03 * k, 0.01))


def added(ks, capacity=64, vs=0.1):
    """A device map after add() of the windows `ks`."""
    import torch
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    m = AccumulatedCloud(vs, DEV, capacity)
    for k in ks:
        pts, mv, stamp, pose = window(k)
        m.add(torch.from_numpy(pts).to(DEV), pose, torch.from_numpy(mv).to(DEV), stamp)
    return m


# ---- the host drivers -------------------------------------------------------------------------------------------------------------------------------
def host_driver_fixture(name, folder):
    """The module-scoped fixture that builds tests/<name>.cpp once, in a temporary folder called `folder`."""
    import pytest
    from helpers import build_host_driver

    @pytest.fixture(scope='module')
    def host_exe(tmp_path_factory):
        return build_host_driver(tmp_path_factory.mktemp(folder), name)
    return host_exe


def map_bytes(keys, acc=None, stamps=None, pierced=None):
    """A map as accum_host.h reads it: i64 keys, i64 acc, i32 stamps, i32 ray counts; a table that is None is left out."""
    raw = np.ascontiguousarray(keys, np.int64).tobytes()
    for table, dtype in ((acc, np.int64), (stamps, np.int32), (pierced, np.int32)):
        if table is not None:
            raw += np.ascontiguousarray(table, dtype).tobytes()
    return raw


def bits(a):
    """A float array as the integers of its bits (+inf, -0.0, nan and every last bit compare as they are); any other array unchanged."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def run_driver(exe, tmp_path, tag, *chunks, suffix='.in'):
    """Writes the chunks (bytes or arrays) to <tag><suffix>, runs the driver (any of its asserts aborts it) and returns the bytes of <tag>.out."""
    src, dst = os.path.join(str(tmp_path), tag + suffix), os.path.join(str(tmp_path), tag + '.out')
    with open(src, 'wb') as f:
        for c in chunks:
            f.write(c if isinstance(c, bytes) else np.ascontiguousarray(c).tobytes())
    subprocess.check_call([exe, src, dst])
    with open(dst, 'rb') as f:
        return f.read()


def unpack(raw, off, layout):
    """Walks (name, dtype, shape) over raw from byte `off` -> ({name: array}, the offset behind the last one); the caller checks that it is the end."""
    out = {}
    for name, dtype, shape in layout:
        n = int(np.prod(shape))
        out[name] = np.frombuffer(raw, dtype, n, off).reshape(shape).copy()
        off += n * np.dtype(dtype).itemsize
    return out, off


def map_layout(rows, sidecar):
    """unpack()'s layout of a map of `rows` rows as accum_host.h writes it."""
    return [('keys', np.int64, (rows,)), ('acc', np.int64, (5, rows)), ('stamps', np.int32, (2, rows)), ('pierced', np.int32, (rows if sidecar else 0,))]


def as_tables(r, pierced):
    """A ReferenceMap and its {key: rays} dict (or None) as the tables a driver returns."""
    keys, acc, stamps = r.records()
    return dict(keys=keys, acc=acc.reshape(5, -1), stamps=stamps.reshape(2, -1), pierced=None if pierced is None else mref.aligned(pierced, keys))


def assert_tables(got, want, what):
    for f in ('keys', 'acc', 'stamps'):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    assert (got['pierced'] is None) == (want['pierced'] is None), what
    assert got['pierced'] is None or np.array_equal(got['pierced'], want['pierced']), what


# ---- device maps ------------------------------------------------------------------------------------------------------------------------------------
def device_cloud(r, pierced=None, pierce_counters=None):
    """The restatement's map as an AccumulatedCloud on the device, through load(); `pierced`: the int32 column beside r.records()' keys, or None."""
    from pcaccumulation_amd.accumulate import AccumulatedCloud
    keys, acc, stamps = r.records()
    extra = {}
    if pierced is not None:
        extra = dict(pierced=pierced, pierce_counters=pierce_counters)
    buf = io.BytesIO()
    np.savez(buf, keys=keys, acc=acc.reshape(5, -1), stamps=stamps.reshape(2, -1), voxel_size=np.float64(r.voxel_size), dropped=np.int64(r.dropped), **extra)
    buf.seek(0)
    return AccumulatedCloud.load(buf, DEV)


def snapshot(m, whole_sidecar=False):
    """Everything a call that leaves the map alone must leave: rows, capacity, dropped, the records and stamps of the rows in use, the ray counts (of
    the rows in use, or the whole tensor), the state words and the pierce counters."""
    n = m.num_voxels
    keys, acc, stamps = m._cur
    pierced = None if m._pierced is None else (m._pierced if whole_sidecar else m._pierced[:n]).clone()
    return (whole_sidecar, n, m.capacity, m.dropped, keys[:n].clone(), acc[:, :n].clone(), stamps[:, :n].clone(), pierced, m._state.clone(),
            None if m._pierce_counters is None else m._pierce_counters.clone())


def assert_unchanged(m, snap, what):
    """The map `m` equals the snapshot, taken to the same extent."""
    import torch
    now = snapshot(m, snap[0])
    assert now[:4] == snap[:4], what
    for a, b in zip(now[4:], snap[4:]):
        assert (a is None and b is None) or torch.equal(a, b), what
