"""Accumulated scene cloud: a voxel map on the device that grows window by window (include/pcacc.h C4).

The test-mode forward returns results['rec_est']: the points of one T-frame window, motion-compensated into the window's anchor frame.
AccumulatedCloud merges a scene's worth of such windows into ONE cloud -- one centroid per occupied voxel, with the number of points, how many of
them were predicted moving, and the first / last time stamp -- without a copy of the points to the host.  All records are integers (fixed-point
coordinate sums), so the map does not depend on the order of the points, on the order of the calls, or on the run.

    m = AccumulatedCloud(voxel_size=0.1, device='cuda')
    for k, (results, input_dict, pose) in enumerate(windows):
        if k:                                                    # refine the (drifting) pose against the map so far: C6, section 9e
            pose = m.register_results(results, input_dict, init_pose=pose, min_count=2, max_moving_fraction=0.0)['pose']
            m.see_through_results(results, input_dict, pose=pose, stamp=k)    # count the rays that pass through the map so far: C7, section 9f
            seen = m.query_results(results, input_dict, pose=pose, max_distance=0.05)   # per point: its voxel's record, nearest centroid: C9, section 9h
            novelty = 1.0 - seen['counters'][native.QUERY_N_OCCUPIED] / seen['counters'][native.QUERY_N_POINTS]   # share of the window the map lacks
        m.add_results(results, input_dict, pose=pose, stamp=k)
        if k % 5 == 4:                                           # every few windows, drop what rays went through, what is 20 windows old and
            x, y, z = pose[:3, 3].tolist()                       # what lies more than 50 m from the sensor: C8, section 9g
            m.prune(min_pierced=2, before_stamp=k - 20, box=((x - 50, y - 50, z - 50), (x + 50, y + 50, z + 50)))
    static = m.extract(min_count=2, max_moving_fraction=0.0)     # dict of device tensors
    keep = m.pierced(min_count=2, max_moving_fraction=0.0) < 2   # rows aligned with `static`: False where later rays went straight through the voxel
    nrm = m.normals(radius=1, min_count=2, max_moving_fraction=0.0, viewpoints=sensor_positions)   # rows aligned with `static` (C5, section 9d)
    image = m.render_range_image(pose, 64, 2048, 0.05, -0.43, max_range=80.0, min_count=2)['depth']   # [64,2048] f64, +inf = nothing there: C10, section 9i
    objects = m.components(min_count=2, max_moving_fraction=0.0, mask=static['points'][:, 2] > ground_z)   # a label per row of `static`, and per connected
                                                                 # set above the ground its size, box and centroid: C11, section 9j
    m.remove_components(min_voxels=30, min_count=2, max_moving_fraction=0.0)   # drop the floating blobs that a per-voxel neighbour count lets through
    m.save_ply('scene.ply', min_count=2, max_moving_fraction=0.0, viewpoints=sensor_positions)
    m.merge(other_session)                                       # another map of the same place on the same grid, exactly as if m had seen its adds: C12,
    m.merge(submap, pose=submap_to_world)                        # section 9l; a map in its own frame or at another voxel size goes through regrid()
    changed = m.compare(last_week, max_distance=0.05)            # per row of extract(), both ways: does the other map hold the voxel, which row, the
    gone = last_week.difference(m, max_distance=0.05)            # nearest centroid within a voxel; what one map has and the other has nothing near, as
    ground = m.select(static['points'][:, 2] < ground_z, min_count=2, max_moving_fraction=0.0)   # a map; any rows of extract() as a map: C13, section 9m
    near = m.knn(scan, k=8, pose=pose, radius=2, min_count=2)    # per point: the rows of extract() and distances of its 8 nearest centroids within
    density = m.neighbors(k=8, radius=2, min_count=2)['mean_distance']   # 2 voxels; the same of every centroid of the map itself: C16, section 9p
    clean = m.select(m.outliers(k=8, std_ratio=2.0, min_count=2)['mask'], invert=True, min_count=2)   # statistical outlier removal, as a new map
    road, objects = clean.split_ground(ground_radius=2, thickness=1)   # what the vehicle stands on and what stands on it, by the local ground under
    image = clean.bev(band=(2, 20))['band_top']                  # every (x, y) column; elevation / ground / obstacle-height images: C17, section 9q
    surfaces = clean.planes(angle=15.0, min_count=2)             # a segment label per row of extract() where neighbouring normals agree, the plane and
    flat, things = clean.split_planes(min_voxels=500, max_rms=0.03, min_count=2)   # rms of every segment; the large flat surfaces and the rest: C18, section 9r
    ground, rest = m.split_ground()                              # the clearance map of a ground robot: the exact (x, y) distance of every column of
    f = rest.distance_field(planar=True, origin=(x0, y0, z_lo), shape=(W, H, band))   # a window to the nearest thing that stands in the robot's height
    free = ~rest.inflate(0.6, field=f)                           # band, and where a robot of radius 0.6 m may be: C19, section 9s

ObservedSpace records, beside a cloud, the voxels the measured rays crossed -- where the sensor looked and found nothing (C14, section 9n).  Filled with
space_now.observe_results(results, input_dict, pose=pose, stamp=k) next to m.add_results(...), it tells what is gone from what was never looked at:

    gone = last_week.difference(m, max_distance=0.05)
    seen = space_now.lookup_voxels(gone.extract()['coords'])
    really_gone = seen['status'] & native.OBSERVED_ENOUGH != 0

Two sessions close the same way on both sides (C15, section 9o): m.merge(other_session) joins the clouds, space_now.merge(other_space) joins the observed
spaces (with pose= when the other session kept its own frame), and space_now.occupancy(m, coords) still answers for the merged map.

There is no CPU path: a CPU tensor raises native.NativeError."""
import math

import numpy as np
import torch

from . import native

_FIELDS = ('points', 'coords', 'count', 'moving', 't_first', 't_last')
_NORMAL_FIELDS = ('normals', 'eigenvalues', 'neighbors', 'flags')
_REGISTER_FIELDS = ('pose', 'fitness', 'rmse', 'iterations', 'status', 'correspondences')
_PRUNE_FIELDS = ('kept', 'filter', 'stale', 'box', 'pierced', 'isolated')
_COMPONENT_FIELDS = ('voxels', 'points', 'moving', 'sum_q', 'centroid', 'lo', 'hi', 't_first', 't_last', 'first_row')
_REMOVE_FIELDS = ('kept', 'small', 'components_removed', 'components_kept', 'rows', 'participating', 'outside', 'masked', 'components', 'largest')
_COMPARE_COUNTERS = ('rows', 'kept', 'same', 'held', 'near', 'only')
_PLY_TYPES = {'float32': 'float', 'float64': 'double', 'int8': 'char', 'uint8': 'uchar', 'int16': 'short', 'uint16': 'ushort', 'int32': 'int',
              'uint32': 'uint'}


def _tables(capacity, device):
    return (torch.empty((capacity,), dtype=torch.int64, device=device),
            torch.empty((native.ACCUM_FIELDS, capacity), dtype=torch.int64, device=device),
            torch.empty((2, capacity), dtype=torch.int32, device=device))


# ---- what the methods that take a scan share: one copy of each check and of each piece of host arithmetic -----------------------------------
def _scan_points(what, name, points, limit, items='points'):
    """points (or targets) is a GPU tensor [n,3] of at most `limit` (a power of two) rows -> n."""
    if not torch.is_tensor(points) or not points.is_cuda:
        raise native.NativeError('%s: %s must be a tensor on the GPU; the HIP path has no CPU fallback' % (what, name))
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError('%s must be [n,3], got %s' % (name, tuple(points.shape)))
    n = points.shape[0]
    if n > limit:
        raise ValueError('at most 2^%d %s per %s, got %d' % (limit.bit_length() - 1, items, what, n))
    return n


def _scan_rows(what, name, t, n):
    """moving or origin_index: None, or [n] on the GPU."""
    if t is not None:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise native.NativeError('%s: %s must live on the GPU' % (what, name))
        if tuple(t.shape) != (n,):
            raise ValueError('%s must be [n], got %s' % (name, tuple(t.shape)))


def _f64(a):
    """A pose, origins or viewpoints: a tensor as it is, an array (or nested lists) as a float64 tensor on the host."""
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _origins(origins):
    """[3] or [S,3], tensor or array -> tensor [S,3], S >= 1."""
    origins = _f64(origins)
    if origins.dim() == 1:
        origins = origins.reshape(1, -1)
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape[0] < 1:
        raise ValueError('origins must be [3] or [S,3] with S >= 1, got %s' % (tuple(origins.shape),))
    return origins


def _origin_rows(origin_index, n_origins):
    if origin_index is None:
        return None
    # the entry point takes int32 rows: a row outside [0, S) stays outside after the cast
    return origin_index.clamp(-1, n_origins).to(torch.int32).contiguous()


def _n_batches(results, input_dict):
    batch = input_dict['time_indice'][:, 0]
    n_batches = results.get('_n_batches')
    if n_batches is None:
        n_batches = int(batch.max()) + 1 if batch.numel() else 1
    return n_batches


def _one_sample(results, input_dict, what):
    n_batches = _n_batches(results, input_dict)
    if n_batches != 1:
        raise ValueError('%s: one sample per batch, got %d' % (what, n_batches))


def _sensor_origins(results, sensor_offset):
    """The sensor position of every frame in the anchor frame: results['ego_motion_est'][0, t] applied to sensor_offset, float64, ((a + b) + c) + d."""
    ego = results['ego_motion_est'][0].detach().to(torch.float64)                       # [T,4,4]
    sx, sy, sz = (float(v) for v in sensor_offset)
    return ((ego[:, :3, 0] * sx + ego[:, :3, 1] * sy) + ego[:, :3, 2] * sz) + ego[:, :3, 3]


def _device_key(device):
    """(type, index) with the index 'cuda' stands for: two maps on 'cuda' and 'cuda:0' share a device."""
    index = device.index
    if index is None and device.type == 'cuda':
        index = torch.cuda.current_device() if torch.cuda.is_available() else 0
    return device.type, index


def _row_mask(what, mask):
    """A mask over the rows of extract() (components, remove_components, select): None, or a 1-D bool / uint8 tensor on the GPU -> uint8, contiguous."""
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dim() != 1 or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError('mask must be a 1-D bool / uint8 tensor over the rows of extract()')
        if not mask.is_cuda:
            raise native.NativeError('%s: mask must live on the GPU; the HIP path has no CPU fallback' % what)
        mask = (mask.to(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()
    return mask


def _bad_mask(rows):
    """The device found a mask whose length is not the number of rows the filter keeps."""
    return ValueError('mask must have one entry per row of extract() under the same filter (%d rows)' % rows)


# ---- the argument checks that several methods make: one copy of each condition and of each message ---------------------------------------------
def _max_distance(max_distance, voxel_size):
    """None = voxel_size -> the float."""
    max_distance = voxel_size if max_distance is None else float(max_distance)
    if not 0.0 < max_distance <= voxel_size:
        raise ValueError('max_distance must lie in (0, voxel_size = %r], got %r' % (voxel_size, max_distance))
    return max_distance


def _margin(margin):
    if not (margin >= 0.0 and np.isfinite(margin)):
        raise ValueError('margin must be a finite number >= 0, got %r' % margin)


def _max_range(max_range):
    if max_range is not None and not float(max_range) >= 0.0:
        raise ValueError('max_range must be >= 0 or None, got %r' % max_range)


def _max_steps(max_steps, limit):
    if not 1 <= int(max_steps) <= limit:
        raise ValueError('max_steps must lie in [1, 2^16], got %r' % max_steps)


def _radius3(radius):
    if not 1 <= int(radius) <= 3:
        raise ValueError('radius must be 1, 2 or 3 voxels, got %r' % radius)


def _min_neighbors3(min_neighbors):
    if int(min_neighbors) < 3:
        raise ValueError('min_neighbors must be at least 3, got %r' % min_neighbors)


def _moving_fraction(max_moving_fraction):
    if max_moving_fraction is not None and np.isnan(float(max_moving_fraction)):
        raise ValueError('max_moving_fraction must be a number or None')


def _stamp32(name, stamp):
    if not -0x80000000 <= int(stamp) <= 0x7fffffff:
        raise ValueError('%s must fit 32 bits, got %r' % (name, stamp))


# ---- voxel keys and boxes of voxel indices ------------------------------------------------------------------------------------------------------
def _voxel_keys(coords):
    """coords [V,3] integers, every index in [-2^20, 2^20) -> C4's keys [V] i64."""
    c = coords.to(torch.int64)
    return ((c[:, 0] + native.ACCUM_IDX_BIAS) << 42) | ((c[:, 1] + native.ACCUM_IDX_BIAS) << 21) | (c[:, 2] + native.ACCUM_IDX_BIAS)


def _voxel_coords(keys):
    """The inverse of _voxel_keys: keys [V] i64 -> coords [V,3] i64."""
    return torch.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1) - native.ACCUM_IDX_BIAS


def _bounding_box(coords, origin):
    """The default window of bev() and distance_field(): index rows [V,k] on the device and the caller's origin or None -> (origin, hi), where a
    None origin becomes the lowest index of every axis and hi is the highest.  A min / max on the device and one read-back; zeros without a row."""
    if coords.shape[0]:
        lo, hi = torch.stack([coords.min(0).values, coords.max(0).values]).tolist()
    else:
        lo = hi = [0] * coords.shape[1]
    return (tuple(lo) if origin is None else origin), hi


class _VoxelTable(object):
    """What AccumulatedCloud and ObservedSpace share: three sorted tables of `capacity` rows on the device, of which the first _n are in use, and
    the protocol by which a call rewrites them.  _cur holds the rows; a call writes its result into _alt, taken at the capacity it needs, and the
    two change places when it has fitted, so that what was there before the call stays in _alt until the next call overwrites it.
    A class sets: _tables(capacity, device) -> the three tensors, keys first; _state_words, the length of _state; _noun, what messages call it."""
    _tables = _state_words = _noun = None

    def __init__(self, voxel_size, device, capacity):
        voxel_size = float(voxel_size)
        if not (voxel_size > 0.0 and np.isfinite(voxel_size)):
            raise ValueError('voxel_size must be a positive finite number, got %r' % voxel_size)
        if not 1 <= int(capacity) <= native.ACCUM_MAX_CAPACITY:
            raise ValueError('capacity must lie in [1, 2^30], got %r' % capacity)
        self.voxel_size = voxel_size
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self._cur = self._alt = self._state = None           # device memory is taken at the first call that needs it
        self._n = 0

    @property
    def num_voxels(self):
        return self._n

    def _ensure(self):
        if self.device.type != 'cuda':
            raise native.NativeError('%s lives on the GPU (got device %s); the HIP path has no CPU fallback' % (type(self).__name__, self.device))
        if self._cur is None:
            self._cur = self._tables(self.capacity, self.device)
            self._state = torch.zeros((self._state_words,), dtype=torch.int64, device=self.device)

    def _pose(self, pose):
        if pose is None:
            return None
        pose = _f64(pose)
        if tuple(pose.shape) != (4, 4):
            raise ValueError('pose must be [4,4], got %s' % (tuple(pose.shape),))
        return pose.to(device=self.device, dtype=torch.float64).contiguous()

    def _box_indices(self, box):
        """(lo [3], hi [3]) in metres of the world frame -> inclusive voxel indices floor(bound / voxel_size), float64 (the map's own division),
        clamped into the grid."""
        try:
            lo, hi = box
            lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        except (TypeError, ValueError):
            raise ValueError('box must be (lo [3], hi [3]) in metres, got %r' % (box,))
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError('box must be (lo [3], hi [3]) in metres, got %r' % (box,))
        if not all(np.isfinite(v) for v in lo + hi):
            raise ValueError('box: every bound must be finite, got %r' % (box,))
        if any(l > h for l, h in zip(lo, hi)):
            raise ValueError('box: lo must not lie above hi, got %r' % (box,))
        grid_lo, grid_hi = float(-native.ACCUM_IDX_BIAS), float(native.ACCUM_IDX_BIAS - 1)
        index = lambda v: int(min(max(np.floor(np.float64(v) / np.float64(self.voxel_size)), grid_lo), grid_hi))
        return [index(v) for v in lo], [index(v) for v in hi]

    # ---- the two sets of tables ----------------------------------------------------------------------------------------------------------
    def _stage(self, capacity):
        """-> self._alt as tables of `capacity` rows: the ones that are there if they have that many, else new ones."""
        if self._alt is None or self._alt[0].shape[0] != capacity:
            self._alt = None                                       # release before taking the other tables
            self._alt = self._tables(capacity, self.device)
        return self._alt

    def _swap(self):
        self._cur, self._alt = self._alt, self._cur                # what was there before the call stays in self._alt, which the next call overwrites

    def _grow(self, what, attempt, described=None, leave=()):
        """A call whose result may have more rows than the capacity: attempt(capacity) launches it from self._cur into self._alt, which has that many
        rows, does its one read-back and returns (status, the rows the result needs, the words it read, with whatever else its caller wants back).
        Until the status is ACCUM_OK the capacity doubles up to what is needed and the attempt is made again; self._cur is untouched by an attempt
        that does not fit.  Then the tables change places and the capacity is the new one.  A status in `leave` ends the call as it stands,
        without either.  -> (status, what the attempt returned third)."""
        capacity = self.capacity
        while True:
            self._stage(capacity)
            status, need, host = attempt(capacity)
            if status == native.ACCUM_OK:
                break
            if status in leave:
                return status, host
            if status != native.ACCUM_TOO_SMALL:
                raise native.NativeError('%s: the state words do not describe the %s (status %d)' % (what, described or self._noun, status))
            if need > native.ACCUM_MAX_CAPACITY:
                raise native.NativeError('%s: the %s would take %d voxels, more than 2^30' % (what, self._noun, need))
            while capacity < need:                                 # growth by doubling
                capacity = min(2 * capacity, native.ACCUM_MAX_CAPACITY)
        self._swap()
        self.capacity = capacity
        return status, host

    # ---- what copy, regrid, select, merge and load share ---------------------------------------------------------------------------------------
    def _copy_rows(self, c):
        """The rows in use and the state words into `c`, a new object of this capacity -> c."""
        c._n = self._n
        if self._cur is not None:
            c._ensure()
            for dst, src in zip(c._cur, self._cur):
                dst[..., :self._n].copy_(src[..., :self._n])
            c._state.copy_(self._state)
        return c

    def _room(self, capacity):
        """The capacity of a result that never has more rows than this one: None = this one's."""
        capacity = self.capacity if capacity is None else int(capacity)
        if capacity < max(self._n, 1):
            raise ValueError('capacity must be at least the %d rows of the %s (the result never has more), got %r' % (self._n, self._noun, capacity))
        return capacity

    def _regrid_args(self, pose, voxel_size, capacity):
        if pose is None and voxel_size is None:
            raise ValueError('regrid needs a pose, a voxel_size or both')
        return self.voxel_size if voxel_size is None else float(voxel_size), self._room(capacity)

    def _peer(self, what, other, kind):
        """`other` is a `kind` on this device."""
        if not isinstance(other, kind):
            raise TypeError('%s takes an %s, got %s' % (what, kind.__name__, type(other).__name__))
        if _device_key(other.device) != _device_key(self.device):
            raise ValueError('%s: the maps live on %s and %s; save() / load() carries a map across' % (what, self.device, other.device))

    def _merge_args(self, other, pose, kind):
        self._peer('merge', other, kind)
        if pose is None and other.voxel_size != self.voxel_size:
            raise ValueError('merge: voxel sizes %r and %r differ; give pose= (np.eye(4) keeps the frame) or regrid() the other map first'
                             % (self.voxel_size, other.voxel_size))

    def _records(self):
        tables = self._tables(0, 'cpu') if self._cur is None or self._n == 0 else self._cur
        return tuple(t[..., :self._n].cpu().numpy() for t in tables)

    @staticmethod
    def _ascending(path, keys):
        if keys.shape[0] and (np.any(keys[1:] <= keys[:-1]) or keys[0] < 0):
            raise ValueError('%s: the keys are not ascending' % path)

    @classmethod
    def _from_records(cls, columns, voxel_size, device):
        """load(): an object whose capacity is 64 doubled until the rows fit, with the host arrays `columns`, keys first, as its rows."""
        m = columns[0].shape[0]
        capacity = 64
        while capacity < m:
            capacity *= 2
        self = cls(voxel_size, device, capacity)
        self._ensure()
        if m:
            for dst, src in zip(self._cur, columns):
                dst[..., :m] = torch.from_numpy(src).to(self.device)
        self._n = m
        return self


class AccumulatedCloud(_VoxelTable):
    _tables, _state_words, _noun = staticmethod(_tables), native.ACCUM_STATE_WORDS, 'map'

    def __init__(self, voxel_size, device='cuda', capacity=1 << 20):
        super(AccumulatedCloud, self).__init__(voxel_size, device, capacity)
        self._dropped = 0
        self._pierced = self._pierce_counters = None          # the sidecar of see_through: taken at its first call

    # ---- state -------------------------------------------------------------------------------------------------------------------------
    @property
    def dropped(self):
        """Points that were not accumulated: a non-finite coordinate, |coordinate| >= 32768 or a voxel index outside +-2^20."""
        return self._dropped

    def clear(self):
        self._n = self._dropped = 0
        self._pierced = self._pierce_counters = None
        if self._state is not None:
            self._state.zero_()

    # ---- add ---------------------------------------------------------------------------------------------------------------------------
    def add(self, points, pose=None, moving=None, stamp=0):
        """points [n,3] f32 (device), pose [4,4] window-to-world (tensor or array; None = identity), moving [n] bool / integer (non-zero = predicted
        moving; None = none), stamp: one integer for the call.  Only the map's eight state words are read back."""
        n = _scan_points('add', 'points', points, native.ACCUM_MAX_POINTS)
        _scan_rows('add', 'moving', moving, n)
        if n == 0:
            return self
        self._ensure()
        pts = points.detach().float().contiguous()
        mv = (moving != 0).to(torch.uint8).contiguous() if moving is not None else None
        pose = self._pose(pose)

        def attempt(capacity):
            native.accum_add(pts, pose, mv, int(stamp), self.voxel_size, self._cur, self._alt, self._state)
            state = self._state.tolist()                           # the one read-back of an add
            return state[native.ACCUM_STATUS], state[native.ACCUM_NEEDED], state
        state = self._grow('accum_add', attempt)[1]
        if self._pierced is not None:                              # carry the sidecar: the old map sits untouched in self._alt
            self._pierced = self._carry(self._pierced, self._alt[0], self._n, self._cur[0], state[native.ACCUM_NUM_VOXELS])
        self._n = state[native.ACCUM_NUM_VOXELS]
        self._dropped = state[native.ACCUM_DROPPED]
        return self

    def add_results(self, results, input_dict, pose=None, stamp=0):
        """A test / val-mode forward: results['rec_est'] with the predicted-moving flag as MotionNet hands it to Cluster
        (results['mos_est'].argmax(1) == 1).  One sample per batch, or one pose per sample ([B,4,4])."""
        points = results['rec_est']
        moving = results['mos_est'].argmax(1) == 1
        if pose is not None:
            pose = _f64(pose)
        if pose is not None and pose.dim() == 3:
            batch = input_dict['time_indice'][:, 0]
            for b in range(pose.shape[0]):
                rows = torch.nonzero(batch == b).reshape(-1)
                self.add(points.index_select(0, rows), pose[b], moving.index_select(0, rows), stamp)
            return self
        n_batches = _n_batches(results, input_dict)
        if n_batches != 1:
            raise ValueError('add_results: %d samples in the batch need one pose per sample, [B,4,4]' % n_batches)
        return self.add(points, pose, moving, stamp)

    @staticmethod
    def _carry(pierced, old_keys, n_old, new_keys, n_new):
        """The sidecar of the merged map: every old key is present among the new ones and keys are below 2^63, so int64 order is key order and
        searchsorted names the new row of every old row.  New voxels start at 0."""
        out = torch.zeros((new_keys.shape[0],), dtype=torch.int32, device=pierced.device)
        if n_old:
            out[torch.searchsorted(new_keys[:n_new], old_keys[:n_old])] = pierced[:n_old]
        return out

    # ---- extract -----------------------------------------------------------------------------------------------------------------------
    def extract(self, min_count=1, max_moving_fraction=None):
        """One row per voxel with count >= min_count and, when max_moving_fraction is given, moving / count <= max_moving_fraction, in
        ascending (x, y, z) voxel order: points [V,3] f32 centroids, coords [V,3] i32, count, moving [V] i64, t_first, t_last [V] i32."""
        self._ensure()
        out = native.accum_extract(self._cur, self._n, min_count, max_moving_fraction)
        kept = int(out[-1]) if self._n else 0
        return {k: t[:kept] for k, t in zip(_FIELDS, out)}

    # ---- normals -----------------------------------------------------------------------------------------------------------------------
    def normals(self, radius=1, min_neighbors=5, min_count=1, max_moving_fraction=None, viewpoints=None, stamp_base=0):
        """One oriented surface normal per voxel that extract(min_count, max_moving_fraction) keeps, row for row (include/pcacc.h C5): the covariance
        of the float64 centroids of the kept voxels within `radius` voxels (Chebyshev, the voxel itself included), its smallest eigenvector.
        -> normals [V,3] f32 (zero where invalid), eigenvalues [V,3] f32 descending, neighbors [V] i32, flags [V] u8 (1: fewer than min_neighbors,
        2: collinear or a single point, 4: oriented towards a viewpoint), valid [V] bool (neither 1 nor 2).
        viewpoints [S,3] (tensor or array): the sensor position of stamp stamp_base + s; a voxel whose first stamp has a row there gets the normal
        that faces it, every other voxel the normal whose first non-zero of (n_z, n_y, n_x) is positive.  Only the kept count is read back."""
        radius, min_neighbors = int(radius), int(min_neighbors)
        _radius3(radius)
        _min_neighbors3(min_neighbors)
        if viewpoints is not None:
            viewpoints = _f64(viewpoints)
            if viewpoints.dim() != 2 or viewpoints.shape[1] != 3:
                raise ValueError('viewpoints must be [S,3], got %s' % (tuple(viewpoints.shape),))
        self._ensure()
        if viewpoints is not None:
            viewpoints = viewpoints.to(device=self.device, dtype=torch.float64).contiguous()
        out = native.accum_normals(self._cur, self._n, min_count, max_moving_fraction, radius, min_neighbors, viewpoints, int(stamp_base))
        kept = int(out[-1]) if self._n else 0
        res = {k: t[:kept] for k, t in zip(_NORMAL_FIELDS, out)}
        res['valid'] = (res['flags'] & (native.NORMAL_FEW_NEIGHBORS | native.NORMAL_DEGENERATE)) == 0
        return res

    # ---- register ----------------------------------------------------------------------------------------------------------------------
    def register(self, points, init_pose=None, moving=None, max_distance=None, max_iter=30, min_count=1, max_moving_fraction=None, radius=1,
                 min_neighbors=5, viewpoints=None, stamp_base=0):
        """Point-to-plane ICP of a scan onto the map (include/pcacc.h C6): the scan-to-world pose to hand to add().  The map is not modified.
        points [n,3] f32 (device), init_pose [4,4] (tensor or array; None = identity), moving [n] (non-zero = predicted moving: the point takes part
        in nothing), max_distance in (0, voxel_size] (None = voxel_size): a point matches the nearest kept centroid with a valid normal among the
        3 x 3 x 3 voxels around it, if within max_distance.  min_count, max_moving_fraction, radius, min_neighbors, viewpoints, stamp_base mean what
        they mean in normals().
        -> dict of device tensors: pose [4,4] f64, fitness, rmse (f64 scalars), iterations, status, correspondences (i32 scalars); status is a sum
        of native.REGISTER_* bits (0 = converged).  Every bit except REGISTER_MAX_ITER leaves fitness and rmse at 0 and the pose at the last good
        value (init_pose when nothing ever matched).
        Every call computes the normals anew, because the rows move with every add: the cost of one normals() call (profiles/accum_normals_bench.txt:
        2.78 ms at 8.0 M voxels and r = 1 without a filter, 1.07 ms with min_count=2, max_moving_fraction=0.0) comes on top of the rounds (profiles/accum_register_bench.txt: about
        2 ms per round at 800 k points against 2 - 8 M voxels).  Only the kept count that normals() reads is read back."""
        n = _scan_points('register', 'points', points, native.REGISTER_MAX_POINTS)
        _scan_rows('register', 'moving', moving, n)
        max_distance = _max_distance(max_distance, self.voxel_size)
        if not 0 <= int(max_iter) <= native.REGISTER_MAX_ITERATIONS:
            raise ValueError('max_iter must lie in [0, %d], got %r' % (native.REGISTER_MAX_ITERATIONS, max_iter))
        init = self._pose(init_pose)
        nrm = self.normals(radius, min_neighbors, min_count, max_moving_fraction, viewpoints, stamp_base)
        pts = points.detach().float().contiguous()
        mv = (moving != 0).to(torch.uint8).contiguous() if moving is not None else None
        out = native.accum_register(pts, mv, init, self.voxel_size, max_distance, int(max_iter), self._cur, self._n, min_count,
                                    max_moving_fraction, nrm['normals'], nrm['flags'])
        return dict(zip(_REGISTER_FIELDS, out))

    def register_results(self, results, input_dict, init_pose=None, **kw):
        """register() of a test / val-mode forward: results['rec_est'], with results['mos_est'].argmax(1) == 1 as `moving`.  One sample per batch."""
        _one_sample(results, input_dict, 'register_results')
        return self.register(results['rec_est'], init_pose, results['mos_est'].argmax(1) == 1, **kw)

    # ---- query -------------------------------------------------------------------------------------------------------------------------
    def query(self, points, pose=None, max_distance=None, min_count=1, max_moving_fraction=None, normals=False, require_normal=False, radius=1,
              min_neighbors=5, viewpoints=None, stamp_base=0):
        """What the map knows at every point of a scan (include/pcacc.h C9).  The map is not modified.
        points [n,3] f32 (device), pose [4,4] scan-to-world (tensor or array; None = identity), max_distance in (0, voxel_size] (None = voxel_size).
        -> dict of device tensors, one row per point in the caller's order:
        status [n] u8, a sum of native.QUERY_* bits: INVALID (the point is not finite or lies outside the grid: every other field at its default),
        OCCUPIED (the map has the point's voxel), KEPT (extract(min_count, max_moving_fraction) returns that voxel), MATCHED, NORMAL;
        count, moving [n] i64, t_first, t_last [n] i32: the record of the point's own voxel, pierced [n] i32: its see_through count (all 0 without one);
        row [n] i32, nearest [n,3] f32, distance [n] f64: the nearest centroid extract(min_count, max_moving_fraction) returns among the 3 x 3 x 3 voxels
        around the point, if within max_distance -- its row there (valid until the next add or prune), extract's point, the distance to the float64
        centroid; -1, 0, +inf without a match.  For max_distance <= 0.9 voxel_size this is the nearest kept centroid of the whole map.
        normals=True computes normals(radius, min_neighbors, ..., viewpoints, stamp_base) under the same filter, as register() does, and adds
        plane_distance [n] f64: the signed distance of the point to the plane through the matched centroid (+inf without a valid normal there);
        require_normal=True matches only centroids with a valid normal: register()'s correspondences.
        counters [7] i64: points, invalid, occupied, kept, matched, with a normal, and native.QUERY_BAD_TABLE (always 0 from here).
        Nothing is read back beyond the kept count normals() reads when normals=True."""
        _scan_points('query', 'points', points, native.QUERY_MAX_POINTS)
        max_distance = _max_distance(max_distance, self.voxel_size)
        _radius3(radius)
        _min_neighbors3(min_neighbors)
        if require_normal and not normals:
            raise ValueError('require_normal=True needs normals=True')
        pose = self._pose(pose)
        self._ensure()
        nrm = flags = None
        if normals:
            res = self.normals(radius, min_neighbors, min_count, max_moving_fraction, viewpoints, stamp_base)
            nrm, flags = res['normals'], res['flags']
        return native.accum_query(points.detach().float().contiguous(), pose, self.voxel_size, max_distance, self._cur, self._n, self._pierced, min_count,
                                  max_moving_fraction, nrm, flags, bool(require_normal) and nrm.shape[0] > 0)   # no kept row: nothing can match

    def query_results(self, results, input_dict, pose=None, **kw):
        """query() of a test / val-mode forward: results['rec_est'].  One sample per batch."""
        _one_sample(results, input_dict, 'query_results')
        return self.query(results['rec_est'], pose, **kw)

    # ---- k nearest ---------------------------------------------------------------------------------------------------------------------
    def _knn_args(self, k, radius, max_distance):
        """k, radius and max_distance (None = radius * voxel_size) as the entry points of C16 take them."""
        k, radius = int(k), int(radius)
        if not 1 <= k <= native.KNN_MAX_K:
            raise ValueError('k must lie in [1, %d], got %r' % (native.KNN_MAX_K, k))
        if not 1 <= radius <= native.KNN_MAX_RADIUS:
            raise ValueError('radius must lie in [1, %d] voxels, got %r' % (native.KNN_MAX_RADIUS, radius))
        reach = radius * self.voxel_size
        max_distance = reach if max_distance is None else float(max_distance)
        if not 0.0 < max_distance <= reach:
            raise ValueError('max_distance must lie in (0, radius * voxel_size = %r], got %r' % (reach, max_distance))
        return k, radius, max_distance

    def knn(self, points, k, pose=None, radius=2, max_distance=None, min_count=1, max_moving_fraction=None):
        """The k nearest centroids of the map for every point of a scan, within `radius` voxels (include/pcacc.h C16).  The map is not modified.
        points [n,3] f32 (device), k in [1, 16], pose [4,4] scan-to-world (tensor or array; None = identity), radius in [1, 4] voxels, max_distance in
        (0, radius * voxel_size] (None = radius * voxel_size).  The candidates are the centroids extract(min_count, max_moving_fraction) returns in the
        (2 radius + 1)^3 voxels around the point's voxel.
        -> dict of device tensors, one row per point in the caller's order: rows [n,k] i32 (the neighbours' rows of that extract(), nearest first, ties
        to the lower row; valid until the next add or prune; -1 = none), distance [n,k] f64 (to the float64 centroid; +inf = none), found [n] i32,
        status [n] u8 (native.KNN_INVALID: the point is not finite or lies outside the grid; else KNN_FOUND with a neighbour, KNN_FULL with k),
        counters [5] i64: queries, invalid, with a neighbour, with k neighbours, neighbours in total.
        For max_distance <= (radius - 0.1) voxel_size these are the k nearest kept centroids of the whole map within max_distance.
        Nothing is read back."""
        _scan_points('knn', 'points', points, native.KNN_MAX_POINTS)
        k, radius, max_distance = self._knn_args(k, radius, max_distance)
        pose = self._pose(pose)
        self._ensure()
        return native.accum_knn(points.detach().float().contiguous(), pose, self.voxel_size, max_distance, k, radius, self._cur, self._n, min_count,
                                max_moving_fraction)

    def knn_results(self, results, input_dict, pose=None, **kw):
        """knn() of a test / val-mode forward: results['rec_est'].  One sample per batch; k goes by keyword."""
        _one_sample(results, input_dict, 'knn_results')
        return self.knn(results['rec_est'], pose=pose, **kw)

    def neighbors(self, k, radius=2, max_distance=None, min_count=1, max_moving_fraction=None):
        """The k nearest other centroids of every centroid extract(min_count, max_moving_fraction) returns, row for row (include/pcacc.h C16, self
        mode): knn()'s rows, distance, found, status and counters with the centroid itself left out, and mean_distance [V] f64, the mean of the found
        distances (+inf without a neighbour): a local density.  Only the kept count is read back."""
        k, radius, max_distance = self._knn_args(k, radius, max_distance)
        self._ensure()
        out = native.accum_knn_self(self.voxel_size, max_distance, k, radius, self._cur, self._n, min_count, max_moving_fraction)
        kept = int(out.pop('kept')) if self._n else 0
        return {name: (t if name == 'counters' else t[:kept]) for name, t in out.items()}

    def outliers(self, k=8, std_ratio=2.0, radius=2, max_distance=None, min_count=1, max_moving_fraction=None):
        """Statistical outlier test of the map itself, rows aligned with extract(min_count, max_moving_fraction): mean_distance [V] f64 of neighbors(k,
        ...), threshold = mean + std_ratio * population standard deviation of its finite entries (float64, on the device; NaN when there is none) and
        mask [V] bool = mean_distance > threshold; a row without a neighbour has +inf and is always an outlier.  Removal is
        select(mask, invert=True, min_count=..., max_moving_fraction=...).  Read back: the kept count and the one scalar."""
        std_ratio = float(std_ratio)
        if not np.isfinite(std_ratio):
            raise ValueError('std_ratio must be finite, got %r' % std_ratio)
        mean = self.neighbors(k, radius, max_distance, min_count, max_moving_fraction)['mean_distance']
        finite = torch.isfinite(mean)
        count = finite.sum()
        total = torch.where(finite, mean, torch.zeros_like(mean)).sum()
        mu = total / count
        var = (torch.where(finite, mean - mu, torch.zeros_like(mean)) ** 2).sum() / count
        threshold = float(mu + std_ratio * torch.sqrt(var))                      # the one scalar; NaN (0 / 0) without a finite entry
        return dict(mean_distance=mean, threshold=threshold, mask=(mean > threshold) | ~finite)

    # ---- columns, ground, bird's-eye view ----------------------------------------------------------------------------------------------
    def _column_args(self, ground_radius, thickness, band, min_count, max_moving_fraction):
        """ground_radius, thickness and band = (lo, hi) as the entry points of C17 take them, and the filter."""
        ground_radius, thickness = int(ground_radius), int(thickness)
        if not 0 <= ground_radius <= native.COLUMNS_MAX_RADIUS:
            raise ValueError('ground_radius must lie in [0, %d] columns, got %r' % (native.COLUMNS_MAX_RADIUS, ground_radius))
        if not 0 <= thickness <= native.COLUMNS_MAX_HEIGHT:
            raise ValueError('thickness must lie in [0, 2^21) voxels, got %r' % thickness)
        if band is None or len(band) != 2:
            raise ValueError('band must be (lo, hi) in voxels above the ground, got %r' % (band,))
        lo, hi = int(band[0]), int(band[1])
        if not 0 <= lo <= hi <= native.COLUMNS_MAX_HEIGHT:
            raise ValueError('band must hold 0 <= lo <= hi < 2^21, got %r' % (band,))
        return ground_radius, thickness, lo, hi, self._filter_args(min_count, max_moving_fraction)

    def columns(self, ground_radius=2, thickness=1, band=(2, 20), min_count=1, max_moving_fraction=None):
        """The (x, y) columns of the voxels extract(min_count, max_moving_fraction) returns, the local ground under each and the height of every
        voxel above it (include/pcacc.h C17).  The map is not modified.  A column is a run of consecutive rows of that extract(), ascending in z.
        ground_radius in [0, 8] columns: the ground of a column is the lowest voxel of the columns within that many columns of it on both axes
        (a minimum filter: it bridges what stands on the ground up to 2 ground_radius columns wide, and undershoots a slope by up to slope x
        ground_radius); thickness in voxels: a voxel is ground when it lies at most that far above the local ground; band = (lo, hi) voxels above it.
        -> dict of device tensors.  Per column, C rows in (x, y) order: key [C] i64 ((x + 2^20) << 21 | (y + 2^20)), xy [C,2] i32, first_row, voxels
        [C] i32 (rows [first_row, first_row + voxels) of extract()), points, moving [C] i64, z_low, z_high [C] i32 (voxel indices), t_first, t_last,
        ground_z [C] i32 (voxel index of the local ground), ground_row (the row of extract() that is it), ground_column (its column; ties go to
        the lower (x, y)), band_voxels (voxels of the column with lo <= z - ground_z <= hi), band_top (the largest such z - ground_z, -1 = none).
        Per row of extract(): row_column [V] i32, row_height [V] i32 = z - ground_z, row_is_ground [V] u8, row_height_m [V] f64 = the float64 z
        centroid minus that of ground_row (slightly negative at most by 2^-16 m).  counters [5] i64: rows, columns, ground rows, rows in the band,
        columns whose ground came from another column.  Clean floaters first (outliers, remove_components, prune): one voxel below the road pulls
        the ground of its neighbourhood down.  Read back: the two counts."""
        ground_radius, thickness, lo, hi, min_count = self._column_args(ground_radius, thickness, band, min_count, max_moving_fraction)
        self._ensure()
        out = native.accum_columns(self._cur, self._n, min_count, max_moving_fraction, ground_radius, thickness, lo, hi)
        n = out.pop('n')
        kept, n_col = n.tolist() if self._n else (0, 0)             # the one read-back
        return {name: (t if name == 'counters' else t[:kept] if name.startswith('row_') else t[:n_col]) for name, t in out.items()}

    def ground_mask(self, **kw):
        """mask [V] bool over the rows of extract() under the same filter: columns(**kw)['row_is_ground'] != 0."""
        return self.columns(**kw)['row_is_ground'] != 0

    def split_ground(self, **kw):
        """(ground, rest): the voxels ground_mask(**kw) names and the others as two NEW maps, through select(); this map is not modified."""
        f = {a: kw[a] for a in ('min_count', 'max_moving_fraction') if a in kw}
        mask = self.ground_mask(**kw)
        return self.select(mask, **f), self.select(mask, invert=True, **f)

    def bev(self, origin=None, shape=None, **column_kw):
        """Bird's-eye-view images of a window of columns (include/pcacc.h C17): origin = (x0, y0) and shape = (H, W) in voxel indices, pixel (r, c) is
        column (x0 + c, y0 + r); None = the bounding box of the columns (a min / max on the device and one more read-back; (0, 0) and (1, 1) for an
        empty map).  column_kw: the arguments of columns().
        -> column [H,W] i32 (the row of the columns() tables, -1 = empty), elevation [H,W] f32 (extract()'s z of the column's top voxel), ground
        [H,W] f32 (that of its ground_row), both NaN where empty, band_top [H,W] i32 (-1), voxels [H,W] i32 (0); origin (x0, y0), voxel_size, and
        columns: the columns() dict the images were made from."""
        if origin is not None and (len(origin) != 2 or not all(abs(int(v)) <= 1 << 31 for v in origin)):
            raise ValueError('origin must be (x0, y0) in voxel indices, got %r' % (origin,))
        if shape is not None and (len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1 or int(shape[0]) * int(shape[1]) > native.BEV_MAX_PIXELS):
            raise ValueError('shape must be (H, W) with H, W >= 1 and at most 2^28 pixels, got %r' % (shape,))
        cols = self.columns(**column_kw)
        f = {a: column_kw[a] for a in ('min_count', 'max_moving_fraction') if a in column_kw}
        if origin is None or shape is None:
            origin, hi = _bounding_box(cols['xy'], origin)          # the one more read-back
            if shape is None:
                shape = (hi[1] - int(origin[1]) + 1, hi[0] - int(origin[0]) + 1)
                if shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] > native.BEV_MAX_PIXELS:
                    raise ValueError('the columns from origin %r on span %r pixels: give a shape of at most 2^28 pixels' % (tuple(origin), shape))
        x0, y0, height, width = int(origin[0]), int(origin[1]), int(shape[0]), int(shape[1])
        out = native.accum_bev(self._cur, self._n, self._filter_args(f.get('min_count', 1), f.get('max_moving_fraction')), f.get('max_moving_fraction'),
                               cols, x0, y0, width, height)
        out.update(origin=(x0, y0), voxel_size=self.voxel_size, columns=cols)
        return out

    # ---- distance field, clearance, inflation ------------------------------------------------------------------------------------------
    def _field_args(self, origin, shape, max_radius, planar, pad, min_count, max_moving_fraction):
        """The arguments of distance_field() checked, before anything is allocated -> (max_radius, min_count)."""
        max_radius = int(max_radius)
        if not 1 <= max_radius <= native.FIELD_MAX_RADIUS:
            raise ValueError('max_radius must lie in [1, %d] voxels, got %r' % (native.FIELD_MAX_RADIUS, max_radius))
        if origin is not None and (len(origin) != 3 or not all(abs(int(v)) <= native.FIELD_MAX_ORIGIN for v in origin)):
            raise ValueError('origin must be (x0, y0, z0) in voxel indices, each at most 2^31 in size, got %r' % (origin,))
        if shape is not None and (len(shape) != 3 or not all(int(v) >= 1 for v in shape)):
            raise ValueError('shape must be (nx, ny, nz) with every side >= 1, got %r' % (shape,))
        if origin is not None and shape is not None:
            self._field_box(origin, shape, max_radius, planar, pad)
        return max_radius, self._filter_args(min_count, max_moving_fraction)

    @staticmethod
    def _field_box(origin, shape, max_radius, planar, pad):
        """The box a call runs on: (origin, shape) grown by max_radius on every side (x and y only when planar) with pad -> (origin, shape, grow)."""
        grow = (max_radius, max_radius, 0 if planar else max_radius) if pad else (0, 0, 0)
        origin = tuple(int(v) - g for v, g in zip(origin, grow))
        shape = tuple(int(v) + 2 * g for v, g in zip(shape, grow))
        if not all(abs(v) <= native.FIELD_MAX_ORIGIN for v in origin):
            raise ValueError('the box%s starts at %r: beyond 2^31' % (' grown by max_radius' if pad else '', origin))
        if shape[0] * shape[1] * (1 if planar else shape[2]) > native.FIELD_MAX_CELLS:
            raise ValueError('the box%s has %r cells: at most 2^28; give a smaller box, a smaller max_radius or pad=False'
                             % (' grown by max_radius' if pad else '', shape))
        return origin, shape, grow

    def _kept_coords(self, min_count, max_moving_fraction):
        """The voxel indices [V,3] i64 of the rows extract's filter keeps, from the keys and the two counts alone: no centroid, no other column."""
        keys, acc, _ = self._cur
        count, moving = acc[0, :self._n], acc[1, :self._n]
        keep = count >= min_count
        if max_moving_fraction is not None:
            keep &= moving.double() / count.double() <= float(max_moving_fraction)
        return _voxel_coords(keys[:self._n][keep])

    def _distance(self, dist2):
        """Metres, f32: sqrt(dist2) * voxel_size in float64, inf where there is no result."""
        metres = torch.sqrt(dist2.clamp(min=0).double()) * self.voxel_size
        return torch.where(dist2 >= 0, metres, torch.full_like(metres, float('inf'))).float()

    def distance_field(self, origin=None, shape=None, max_radius=32, planar=False, pad=True, min_count=1, max_moving_fraction=None):
        """How far every voxel of a box is from the nearest voxel extract(min_count, max_moving_fraction) returns, exactly, up to max_radius voxels,
        and which voxel that is (include/pcacc.h C19).  The map is not modified.  origin = (x0, y0, z0) and shape = (nx, ny, nz) in voxel indices;
        None = the bounding box of the kept voxels (a min / max on the device and one read-back; (0, 0, 0) and (1, 1, 1) for an empty map).
        max_radius in [1, 128] voxels.  planar: distances in (x, y) only, to any kept voxel with z inside [z0, z0 + nz): one plane, the clearance map
        of a ground vehicle.  pad: the call runs on the box grown by max_radius on every side (x and y only when planar) and returns the inner part,
        so that voxels just outside the box count; the counters are then those of the GROWN box, and the limit of 2^28 cells applies to it.
        -> dict: dist2 [nx, ny, nz or 1] i32, the squared distance in voxels, -1 where nothing lies within max_radius; nearest, same shape, i32, the
        row of extract() under the same filter that is nearest (ties go to the lowest row), -1 likewise; distance f32 = sqrt(dist2) * voxel_size in
        metres, inf where -1; origin, shape, planar, max_radius, voxel_size; counters [4] i64: kept rows, sites (voxels inside the box; planar:
        columns that hold one), cells with a result, cells without one."""
        max_radius, min_count = self._field_args(origin, shape, max_radius, planar, pad, min_count, max_moving_fraction)
        self._ensure()
        if origin is None or shape is None:
            origin, hi = _bounding_box(self._kept_coords(min_count, max_moving_fraction), origin)       # the one read-back
            if shape is None:
                shape = tuple(h - int(o) + 1 for h, o in zip(hi, origin))
                if min(shape) < 1:
                    raise ValueError('the kept voxels end before origin %r: give a shape' % (tuple(origin),))
        origin, shape = tuple(int(v) for v in origin), tuple(int(v) for v in shape)
        box_origin, box_shape, grow = self._field_box(origin, shape, max_radius, planar, pad)
        out = native.accum_field(self._cur, self._n, min_count, max_moving_fraction, box_origin, box_shape, max_radius, planar)
        nz_out = 1 if planar else shape[2]
        inner = tuple(slice(g, g + n) for g, n in zip(grow, (shape[0], shape[1], nz_out)))
        dist2, nearest = out['dist2'][inner].contiguous(), out['nearest'][inner].contiguous()
        return dict(dist2=dist2, nearest=nearest, distance=self._distance(dist2), origin=origin, shape=shape, planar=bool(planar), max_radius=max_radius,
                    voxel_size=self.voxel_size, counters=out['counters'])

    def clearance(self, points=None, coords=None, pose=None, field=None, **field_kw):
        """The distance field at the voxels of a scan or at voxel index rows: exactly one of points [n,3] f32 (device; through pose [4,4], None =
        identity) and coords [n,3] int32 / int64 (device).  field: a distance_field() dict to look up in; None = distance_field(**field_kw) first.
        -> dict of device tensors, one row each: status [n] u8, a sum of native.FIELD_VALID (finite and inside the grid), FIELD_INSIDE (the voxel
        lies in the field's box; planar: z inside [z0, z0 + nz)) and FIELD_NEAR (its cell has a result); dist2, row [n] i32, -1 unless NEAR;
        distance [n] f32 in metres, inf unless NEAR; counters [4] i64: rows, valid, inside, near.  Nothing is read back."""
        if (points is None) == (coords is None):
            raise ValueError('clearance: exactly one of points and coords')
        if points is not None:
            _scan_points('clearance', 'points', points, native.ACCUM_MAX_POINTS)
        else:
            _scan_points('clearance', 'coords', coords, native.ACCUM_MAX_POINTS, 'rows')
            if coords.dtype not in (torch.int32, torch.int64):
                raise ValueError('coords must be int32 or int64 voxel indices, got %s' % coords.dtype)
        pose = self._pose(pose)
        if field is None:
            field = self.distance_field(**field_kw)
        elif field_kw:
            raise ValueError('clearance: a field and arguments for a new one: %r' % sorted(field_kw))
        self._ensure()
        if points is not None:
            points = points.detach().float().contiguous()
        else:
            if coords.dtype == torch.int64:                        # an index outside the grid stays outside after the cast
                coords = coords.clamp(-native.ACCUM_IDX_BIAS - 1, native.ACCUM_IDX_BIAS)
            coords = coords.to(torch.int32).contiguous()
        out = native.accum_field_lookup(points, coords, pose, field['voxel_size'], field['origin'], field['shape'], field['planar'], field['dist2'],
                                        field['nearest'])
        out['distance'] = self._distance(out['dist2'])
        return out

    def inflate(self, radius_m, field=None, **field_kw):
        """The cells of a distance field within radius_m metres of a voxel of the map, as a bool tensor of the field's shape: dist2 >= 0 and dist2 <=
        floor(radius_m / voxel_size)^2.  With the planar field of what stands on the ground, ~inflate(r) is where a vehicle of radius r may be.
        field: a distance_field() dict; None = distance_field(**field_kw).  The radius in voxels must not exceed the field's max_radius."""
        radius_m = float(radius_m)
        if not (radius_m >= 0.0 and np.isfinite(radius_m)):
            raise ValueError('radius_m must be a finite number >= 0, got %r' % radius_m)
        r = int(math.floor(radius_m / self.voxel_size))
        if field is None:
            field = self.distance_field(**field_kw)
        elif field_kw:
            raise ValueError('inflate: a field and arguments for a new one: %r' % sorted(field_kw))
        if r > field['max_radius']:                               # the field knows nothing beyond its max_radius: such cells would pass for free
            raise ValueError('radius_m is %d voxels: above the max_radius %d of the field' % (r, field['max_radius']))
        return (field['dist2'] >= 0) & (field['dist2'] <= r * r)

    # ---- see through -------------------------------------------------------------------------------------------------------------------
    def see_through(self, points, origins, origin_index=None, pose=None, moving=None, stamp=None, margin=None, max_range=None, max_steps=4096):
        """Count, for every voxel of the map, the measured rays of a scan that pass straight through it (include/pcacc.h C7): a voxel that was occupied
        and that later rays pierce was not static, whatever `moving` said when it was filled.  The map's records are not modified.
        points [n,3] f32 (device, scan frame); origins [3] or [S,3] (tensor or array, scan frame): sensor positions; origin_index [n] integers (device;
        None = row 0): the origin of every point; pose [4,4] scan-to-world (None = identity); moving [n] (non-zero = predicted moving: the network
        has moved the point, its ray is skipped); stamp: with one, a voxel counts only when t_last < stamp or t_first > stamp (it was not being filled
        at that time); margin (None = 2 voxel_size): the ray stops this far in front of the point it measured; max_range: rays are cut there;
        max_steps in [1, 2^16]: the most voxels one ray visits.
        Adds to a sidecar, int32 per row of the map, that add() carries along, and -> the counters (rays walked, dropped, skipped, truncated, hits)
        as one int64 device tensor, cumulative since clear().  Nothing is read back."""
        n = _scan_points('see_through', 'points', points, native.ACCUM_MAX_POINTS)
        _scan_rows('see_through', 'moving', moving, n)
        _scan_rows('see_through', 'origin_index', origin_index, n)
        origins = _origins(origins)
        margin = 2.0 * self.voxel_size if margin is None else float(margin)
        _margin(margin)
        _max_range(max_range)
        _max_steps(max_steps, native.PIERCE_MAX_STEPS)
        pose = self._pose(pose)
        self._ensure()
        if self._pierced is None:
            self._pierced = torch.zeros((self.capacity,), dtype=torch.int32, device=self.device)
            self._pierce_counters = torch.zeros((native.PIERCE_COUNTERS,), dtype=torch.int64, device=self.device)
        native.accum_pierce(points.detach().float().contiguous(), (moving != 0).to(torch.uint8).contiguous() if moving is not None else None,
                            origins.to(device=self.device, dtype=torch.float64).contiguous(), _origin_rows(origin_index, origins.shape[0]), pose,
                            self.voxel_size, margin, max_range, stamp, int(max_steps), self._cur, self._n, self._pierced, self._pierce_counters)
        return self._pierce_counters.clone()

    def see_through_results(self, results, input_dict, pose=None, sensor_offset=(0, 0, 0), **kw):
        """see_through() of a test / val-mode forward: the points are results['rec_est'] with results['mos_est'].argmax(1) == 1 as `moving`, the origin of
        a point is the sensor position of its frame (input_dict['time_indice'][:, 1]) in the anchor frame, results['ego_motion_est'][0, t] applied to
        sensor_offset (the sensor in its own frame).  One sample per batch."""
        _one_sample(results, input_dict, 'see_through_results')
        return self.see_through(results['rec_est'], _sensor_origins(results, sensor_offset), input_dict['time_indice'][:, 1], pose, results['mos_est'].argmax(1) == 1, **kw)

    # ---- raycast -----------------------------------------------------------------------------------------------------------------------
    def raycast(self, targets, origins, origin_index=None, pose=None, max_range=None, min_range=0.0, margin=0.0, min_count=1, max_moving_fraction=None,
                max_steps=4096):
        """Looking from an origin towards a target: the first voxel extract(min_count, max_moving_fraction) returns along the ray, and how far away it
        is (include/pcacc.h C10).  The map is not modified.
        targets [n,3] f32 (device, caller's frame); origins [3] or [S,3] (tensor or array, caller's frame); origin_index [n] integers (device; None =
        row 0); pose [4,4] caller's frame to world (None = identity).  With max_range the ray runs that far along its direction, past its target if
        need be; with max_range=None it ends margin in front of the target (see_through's ray).  Voxels the ray enters before min_range are passed
        over; max_steps in [1, 2^16]: the most voxels one ray visits.
        -> dict of device tensors, one row per ray in the caller's order:
        status [n] u8: native.RAYCAST_MISS, _HIT, _TRUNCATED (max_steps voxels without a hit), _SKIPPED (a ray of no length, or min_range >= its
        end), _DROPPED (an end point that is not finite or lies outside the grid, or an origin_index outside [0, S));
        row [n] i32: the hit voxel's row of extract(min_count, max_moving_fraction), valid until the next add or prune; coords [n,3] i32 its voxel,
        point [n,3] f32 its centroid (extract's point); range_in [n] f64: where the ray enters that voxel; depth [n] f64: the centroid's range
        along the ray, within sqrt(3) voxel_size + 2^-17 of range_in; length [n] f64: origin to target; visits [n] i32: voxels visited.
        Without a hit row = -1, coords = point = 0 and range_in = depth = +inf.
        counters [7] i64: rays, dropped, skipped, hit, missed, truncated, visits of all rays.  Nothing is read back."""
        n = _scan_points('raycast', 'targets', targets, native.RAYCAST_MAX_RAYS, 'rays')
        _scan_rows('raycast', 'origin_index', origin_index, n)
        origins = _origins(origins)
        min_range, margin = float(min_range), float(margin)
        if not (min_range >= 0.0 and np.isfinite(min_range)):
            raise ValueError('min_range must be a finite number >= 0, got %r' % min_range)
        _margin(margin)
        if max_range is not None:
            max_range = float(max_range)
            _max_range(max_range)
            if margin != 0.0:
                raise ValueError('margin is measured from the target: it cannot be combined with a max_range')
        _max_steps(max_steps, native.RAYCAST_MAX_STEPS)
        pose = self._pose(pose)
        self._ensure()
        return native.accum_raycast(targets.detach().float().contiguous(), origins.to(device=self.device, dtype=torch.float64).contiguous(),
                                    _origin_rows(origin_index, origins.shape[0]), pose, self.voxel_size, min_range, max_range, margin, int(max_steps), self._cur, self._n, min_count, max_moving_fraction)

    def raycast_results(self, results, input_dict, pose=None, sensor_offset=(0, 0, 0), **kw):
        """raycast() of a test / val-mode forward: the targets are results['rec_est'], the origin of a target is the sensor position of its frame, built
        as see_through_results builds it.  One sample per batch."""
        _one_sample(results, input_dict, 'raycast_results')
        return self.raycast(results['rec_est'], _sensor_origins(results, sensor_offset), input_dict['time_indice'][:, 1], pose, **kw)

    def render_range_image(self, pose, height, width, fov_up, fov_down, max_range, **kw):
        """A range image of the map from a sensor at `pose` ([4,4] sensor-to-world; None = identity): one ray per pixel from the sensor's origin.  Row r
        looks at elevation fov_up - (r + 0.5)(fov_up - fov_down) / height, column c at azimuth pi - (c + 0.5) 2 pi / width (radians; the image's
        middle column looks along +x), direction (cos el cos az, cos el sin az, sin el), computed on the host in float64 and cast to float32.
        -> raycast(directions, (0, 0, 0), pose=pose, max_range=max_range, **kw) with every column reshaped to [height, width, ...] (depth is the range
        image; +inf where nothing was hit) and 'directions' [height, width, 3] f32."""
        height, width = int(height), int(width)
        if height < 1 or width < 1 or height * width > native.RAYCAST_MAX_RAYS:
            raise ValueError('height and width must be at least 1 and height * width at most 2^30, got %r x %r' % (height, width))
        fov_up, fov_down = float(fov_up), float(fov_down)
        if not (np.isfinite(fov_up) and np.isfinite(fov_down)):
            raise ValueError('fov_up and fov_down must be finite, got %r %r' % (fov_up, fov_down))
        if max_range is None:
            raise ValueError('render_range_image needs a max_range: a direction has no target to stop at')
        el = fov_up - (np.arange(height, dtype=np.float64) + 0.5) * (fov_up - fov_down) / height
        az = np.pi - (np.arange(width, dtype=np.float64) + 0.5) * 2.0 * np.pi / width
        d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                      np.sin(el)[:, None] * np.ones_like(az)[None, :]], -1).astype(np.float32)
        directions = torch.from_numpy(d).to(self.device)
        res = self.raycast(directions.reshape(-1, 3), np.zeros((1, 3)), None, pose, max_range, **kw)
        out = {k: (v if k == 'counters' else v.reshape((height, width) + tuple(v.shape[1:]))) for k, v in res.items()}
        out['directions'] = directions
        return out

    def pierced(self, min_count=1, max_moving_fraction=None):
        """[V] int32: the rays see_through counted through every voxel that extract(min_count, max_moving_fraction) returns, row for row; all zeros before
        any see_through.  A key join: extract's coords -> keys -> their rows in the map."""
        coords = self.extract(min_count, max_moving_fraction)['coords']
        if self._pierced is None or coords.shape[0] == 0:
            return torch.zeros((coords.shape[0],), dtype=torch.int32, device=self.device)
        return self._pierced[torch.searchsorted(self._cur[0][:self._n], _voxel_keys(coords))]

    # ---- prune -------------------------------------------------------------------------------------------------------------------------
    def _rewrite(self, dry_run, launch):
        """What prune() and remove_components() share: a call that leaves rows out at the present capacity.  launch(tables_out, pierced_out, state)
        -- all None when dry_run -- runs it and -> its counters as a dict with 'kept'.  Afterwards the tables change places, the ray counts are
        the new ones and 'kept' rows are in use."""
        out = pierced_out = None
        if not dry_run:
            out = self._stage(self.capacity)
            if self._pierced is not None:
                pierced_out = torch.zeros((self.capacity,), dtype=torch.int32, device=self.device)
        res = launch(out, pierced_out, None if dry_run else self._state)
        if not dry_run and self._n:                                # the map before the call stays in self._alt, which the next add overwrites
            self._swap()
            if self._pierced is not None:
                self._pierced = pierced_out
            self._n = res['kept']
        return res

    def prune(self, min_pierced=None, pierced_ratio=None, before_stamp=None, min_count=1, max_moving_fraction=None, box=None, min_neighbors=None,
              radius=1, dry_run=False):
        """Remove rows from the map, on the device (include/pcacc.h C8).  A row leaves for the first reason that holds:
        filter: extract(min_count, max_moving_fraction) would not return it; stale: its last stamp is below before_stamp; box: its voxel lies outside
        box = (lo [3], hi [3]), metres of the world frame, both faces' voxels included; pierced: see_through counted at least min_pierced rays through
        it and, with pierced_ratio, rays / count > pierced_ratio (a wall of 1000 points outlives two grazing rays; without a see_through nothing leaves
        for this reason).  Then, with min_neighbors, isolated: fewer than min_neighbors of the rows that are left so far lie within `radius` voxels
        (1, 2 or 3; Chebyshev, the voxel itself included) -- one pass, not iterated.
        The surviving records are unchanged, and extract, normals, register, pierced, save and save_ply see the pruned map.  The capacity stays.
        -> {'kept', 'filter', 'stale', 'box', 'pierced', 'isolated'}: Python integers that sum to the rows before the call -- the one read-back.
        dry_run=True counts and changes nothing."""
        min_pierced = 0 if min_pierced is None else int(min_pierced)
        min_neighbors = 0 if min_neighbors is None else int(min_neighbors)
        radius, min_count = int(radius), int(min_count)
        if min_pierced < 0 or min_pierced > 0x7fffffff:
            raise ValueError('min_pierced must be None or lie in [0, 2^31), got %r' % min_pierced)
        if pierced_ratio is not None:
            if min_pierced < 1:
                raise ValueError('pierced_ratio needs min_pierced >= 1')
            if not float(pierced_ratio) >= 0.0:
                raise ValueError('pierced_ratio must be >= 0, got %r' % pierced_ratio)
        if before_stamp is not None:
            _stamp32('before_stamp', before_stamp)
        _moving_fraction(max_moving_fraction)
        if not 0 <= min_neighbors <= native.PRUNE_MAX_NEIGHBORS:
            raise ValueError('min_neighbors must be None or lie in [0, %d], got %r' % (native.PRUNE_MAX_NEIGHBORS, min_neighbors))
        if min_neighbors:
            _radius3(radius)
        if box is not None:
            box = self._box_indices(box)
        self._ensure()
        counters = torch.empty((native.PRUNE_COUNTERS,), dtype=torch.int64, device=self.device)

        def launch(out, pierced_out, state):
            native.accum_prune(self._cur, self._n, self._pierced, min_count, max_moving_fraction, before_stamp, box, min_pierced, pierced_ratio,
                               min_neighbors, radius, dry_run, out, pierced_out, counters, state)
            return dict(zip(_PRUNE_FIELDS, counters.tolist()))     # the one read-back of a prune
        return self._rewrite(dry_run, launch)

    # ---- connected components ----------------------------------------------------------------------------------------------------------
    def _components_args(self, what, radius, min_count, max_moving_fraction, mask):
        radius, min_count = int(radius), int(min_count)
        _radius3(radius)
        _moving_fraction(max_moving_fraction)
        return radius, min_count, _row_mask(what, mask)

    @staticmethod
    def _components_status(counters):
        status = counters[native.COMPONENTS_STATUS]
        if status == native.COMPONENTS_BAD_MASK:
            raise _bad_mask(counters[native.COMPONENTS_ROWS] - counters[native.COMPONENTS_OUTSIDE])
        if status != native.COMPONENTS_OK:
            raise native.NativeError('accum_components: a join was abandoned under contention (status %d); the labels are not valid' % status)

    def components(self, radius=1, min_count=1, max_moving_fraction=None, mask=None):
        """Which voxels belong together (include/pcacc.h C11).  The voxels extract(min_count, max_moving_fraction) keeps -- with mask [V] bool / uint8
        (device) over its rows: those whose entry is non-zero -- are joined when they lie within `radius` voxels of each other (1, 2 or 3; Chebyshev);
        the connected sets are numbered 0 .. K-1 in ascending order of their smallest (x, y, z) voxel.
        -> label [V] i32 aligned with extract (-1 where the mask excludes the row); per component voxels [K] i32, points, moving [K] i64 (sums of count
        and moving), sum_q [K,3] i64 (the records' fixed-point coordinate sums), centroid [K,3] f32, lo, hi [K,3] i32 (box in voxel indices, inclusive), t_first, t_last [K] i32, first_row [K] i32 (extract row
        of the smallest voxel); counters [7] i64: native.COMPONENTS_*.  Device tensors; only the counters are read back.  The map is not modified."""
        radius, min_count, mask = self._components_args('components', radius, min_count, max_moving_fraction, mask)
        self._ensure()
        res = native.accum_components(self._cur, self._n, min_count, max_moving_fraction, mask, radius)
        counters = res['counters'].tolist()                        # the one read-back
        self._components_status(counters)
        kept, k = counters[native.COMPONENTS_ROWS] - counters[native.COMPONENTS_OUTSIDE], counters[native.COMPONENTS_K]
        out = {name: res[name][:k] for name in _COMPONENT_FIELDS}
        out['label'] = res['label'][:kept]
        out['counters'] = res['counters']
        return out

    def remove_components(self, min_voxels=None, min_points=None, radius=1, min_count=1, max_moving_fraction=None, mask=None, dry_run=False):
        """Remove the small connected sets from the map, on the device (include/pcacc.h C11): every voxel that takes part in components(radius,
        min_count, max_moving_fraction, mask) and whose component has fewer than min_voxels voxels or fewer than min_points points.  Voxels that do
        not take part (outside the filter or the mask) stay: prune() applies a filter.  The surviving records and ray counts are unchanged.
        -> {'kept', 'small', 'components_removed', 'components_kept', 'rows', 'participating', 'outside', 'masked', 'components', 'largest'}: Python
        integers -- the one read-back.  dry_run=True counts and changes nothing."""
        if min_voxels is None and min_points is None:
            raise ValueError('remove_components needs min_voxels or min_points')
        min_voxels = 0 if min_voxels is None else int(min_voxels)
        min_points = 0 if min_points is None else int(min_points)
        if min_voxels < 0 or min_points < 0:
            raise ValueError('min_voxels and min_points must not be negative, got %r %r' % (min_voxels, min_points))
        radius, min_count, mask = self._components_args('remove_components', radius, min_count, max_moving_fraction, mask)
        self._ensure()
        counters = torch.empty((native.COMPONENTS_COUNTERS + native.COMPONENTS_REMOVE_COUNTERS,), dtype=torch.int64, device=self.device)
        first = native.accum_components(self._cur, self._n, min_count, max_moving_fraction, mask, radius, counters=counters[:native.COMPONENTS_COUNTERS])

        def launch(out, pierced_out, state):
            native.accum_remove_components(self._cur, self._n, self._pierced, min_count, max_moving_fraction, first, min_voxels, min_points, dry_run,
                                           out, pierced_out, counters[native.COMPONENTS_COUNTERS:], state)
            host = counters.tolist()                               # the one read-back, of both stages
            self._components_status(host)                          # a stage that did not end OK has left the tables and the state word alone
            return dict(zip(_REMOVE_FIELDS, host[native.COMPONENTS_COUNTERS:] + host[:native.COMPONENTS_STATUS]))
        return self._rewrite(dry_run, launch)

    # ---- planar segments ---------------------------------------------------------------------------------------------------------------
    def planes(self, angle=15.0, max_offset=None, max_variation=0.01, radius=1, normal_radius=2, min_neighbors=5, min_count=1,
               max_moving_fraction=None, mask=None, normals=None):
        """Which voxels lie on one surface (include/pcacc.h C18): region growing over the voxels extract(min_count, max_moving_fraction) keeps.  A
        voxel takes part when the mask (as for components) names it, its normal is valid and its neighbourhood is flat: the smallest eigenvalue
        of normals() is at most max_variation (in [0, 1]) times the sum of the three.  Two such voxels within `radius` voxels (1, 2 or 3) are
        joined when their normals are within `angle` degrees (in [0, 90], up to sign) and each centroid lies within max_offset metres (None = half
        a voxel) of the other's tangent plane.  The connected sets are numbered 0 .. K-1 by their smallest (x, y, z) voxel.
        normals: an earlier normals() result under the same filter, to be reused; otherwise normals(radius=normal_radius, min_neighbors=...) runs.
        -> label [V] i32 aligned with extract (-1 where the row does not take part), distance [V] f64 (signed, to the plane of the row's own
        segment); per segment voxels [K] i32, points [K] i64, lo, hi [K,3] i32, first_row, t_first, t_last [K] i32, anchor [K,3] i32, spread [K]
        i64, shift [K] i32, s1 [K,3], s2 [K,6] i64 (the integer moments the plane is fitted to), normal, eigenvalues, centroid [K,3] f64, offset,
        mse, rms = sqrt(mse) [K] f64, flags [K] u8 (native.PLANE_DEGENERATE: fewer than three voxels that are not collinear; normal, offset, mse
        and every distance are then 0); counters [9] i64: native.PLANES_*.  Device tensors; only the counters are read back.  The map is not
        modified.  Region growing is single linkage: without the flatness gate (max_variation=1) a chain of slowly turning normals joins two
        surfaces; with it the voxels along creases and edges take no part."""
        radius, min_count, mask = self._components_args('planes', radius, min_count, max_moving_fraction, mask)
        angle, max_variation = float(angle), float(max_variation)
        max_offset = 0.5 * self.voxel_size if max_offset is None else float(max_offset)
        if not 0.0 <= angle <= 90.0:
            raise ValueError('angle must lie in [0, 90] degrees, got %r' % angle)
        if not max_offset >= 0.0:
            raise ValueError('max_offset must be a distance in metres, not negative, got %r' % max_offset)
        if not 0.0 <= max_variation <= 1.0:
            raise ValueError('max_variation must lie in [0, 1], got %r' % max_variation)
        if normals is not None and not (isinstance(normals, dict) and all(torch.is_tensor(normals.get(k)) for k in ('normals', 'eigenvalues', 'flags'))):
            raise ValueError('normals must be a result of normals(): a dict with normals, eigenvalues and flags')
        cos_angle = math.cos(math.radians(angle))                  # formed here and passed as the double: 90 degrees is 6.1e-17, not 0
        self._ensure()
        if normals is None:
            normals = self.normals(radius=normal_radius, min_neighbors=min_neighbors, min_count=min_count, max_moving_fraction=max_moving_fraction)
        res = native.accum_planes(self._cur, self._n, min_count, max_moving_fraction, normals['normals'], normals['eigenvalues'], normals['flags'],
                                  mask, radius, cos_angle, max_offset, max_variation)
        counters = res['counters'].tolist()                        # the one read-back
        status = counters[native.PLANES_STATUS]
        kept, k = counters[native.PLANES_ROWS] - counters[native.PLANES_OUTSIDE], counters[native.PLANES_K]
        if status == native.PLANES_BAD_ROWS:
            raise ValueError('normals and mask must have one row per row of extract() under the same filter (%d rows)' % kept)
        if status != native.PLANES_OK:
            raise native.NativeError('accum_planes: a join was abandoned under contention (status %d); the labels are not valid' % status)
        out = {name: res[name][:k] for name, _, _ in native.PLANES_FIELDS}
        out.update({name: res[name][:kept] for name, _, _ in native.PLANES_ROW_FIELDS})
        out['rms'] = out['mse'].sqrt()
        out['counters'] = res['counters']
        return out

    def plane_mask(self, min_voxels, max_rms=None, **kw):
        """mask [V] bool over the rows of extract() under the same filter: the rows of the segments of planes(**kw) that have a plane, at least
        min_voxels voxels and, with max_rms (metres), rms <= max_rms."""
        res = self.planes(**kw)
        good = ((res['flags'] & native.PLANE_DEGENERATE) == 0) & (res['voxels'] >= int(min_voxels))
        if max_rms is not None:
            good = good & (res['rms'] <= float(max_rms))
        label = res['label'].long()
        return (label >= 0) & good[label.clamp(min=0)] if good.shape[0] else torch.zeros_like(label, dtype=torch.bool)

    def split_planes(self, min_voxels, max_rms=None, **kw):
        """(planar, rest): the voxels plane_mask(min_voxels, max_rms, **kw) names and the others as two NEW maps, through select(); this map is
        not modified."""
        f = {a: kw[a] for a in ('min_count', 'max_moving_fraction') if a in kw}
        mask = self.plane_mask(min_voxels, max_rms, **kw)
        return self.select(mask, **f), self.select(mask, invert=True, **f)

    # ---- merge, regrid, copy -----------------------------------------------------------------------------------------------------------
    def copy(self):
        """An independent clone: device copies of the rows in use, of the ray counts and of the state words.  merge() mutates its map, so
        `c = a.copy(); c.merge(b)` keeps a."""
        c = self._copy_rows(self._like(self.voxel_size, self.capacity))
        c._dropped = self._dropped
        if self._pierced is not None:
            c._pierced[:self._n].copy_(self._pierced[:self._n])
        return c

    def _like(self, voxel_size, capacity):
        """A new, empty map on this device, with ray counts (all 0) and this map's see_through counters if this map has them.  The constructor
        checks voxel_size and capacity; device memory for the tables is taken by the caller's _ensure()."""
        new = AccumulatedCloud(voxel_size, self.device, capacity)
        if self._pierced is not None:
            new._pierced = torch.zeros((capacity,), dtype=torch.int32, device=self.device)
            new._pierce_counters = self._pierce_counters.clone()
        return new

    def _regrid(self, pose, voxel_size, capacity):
        """-> (the new map, the counters of the call as Python integers: the one read-back)."""
        voxel_size, capacity = self._regrid_args(pose, voxel_size, capacity)
        new = self._like(voxel_size, capacity)
        pose = self._pose(pose)
        self._ensure()
        new._ensure()
        counters = torch.empty((native.REGRID_COUNTERS,), dtype=torch.int64, device=self.device)
        native.accum_regrid(self._cur, self._n, self._pierced, pose, voxel_size, self._dropped, new._cur, new._pierced, counters, new._state)
        host = counters.tolist()                                   # the one read-back of a regrid
        new._n = host[native.REGRID_ROWS_OUT]
        new._dropped = self._dropped + host[native.REGRID_DROPPED_POINTS]
        return new, host

    def regrid(self, pose=None, voxel_size=None, capacity=None):
        """This map under a rigid pose ([4,4] map-to-new-frame, tensor or array) and / or at another voxel size, as a NEW AccumulatedCloud on the same
        device (include/pcacc.h C12); this map is not modified.  LOSSY by design: a voxel is treated as `count` points at its centroid, so points
        that the new grid would separate stay together.  Counts, moving counts, stamps (min / max) and ray counts (clamped at 2^31 - 1) are summed per
        new voxel.  A row whose centroid leaves the grid (or is not finite under the pose) is dropped, never clamped: its points are added to the
        new map's `dropped`.  capacity (None = this map's) must hold this map's rows.  Only the five counters are read back."""
        return self._regrid(pose, voxel_size, capacity)[0]

    def merge(self, other, pose=None):
        """Take another map's voxels into this one, on the device (include/pcacc.h C12); `other` is not modified.
        pose=None is the exact path: both maps on one grid (other.voxel_size == self.voxel_size, the same device), and the result is, bit for bit, the
        map one AccumulatedCloud would hold had it been given every add of both: counts, moving counts and coordinate sums added, first stamp the
        minimum, last stamp the maximum, ray counts added (clamped at 2^31 - 1), `dropped` added.  With a pose ([4,4] other-to-world, tensor or array)
        `other` is first regridded under it onto this map's voxel size (regrid: lossy by design) and the result merged.
        The capacity grows as in add().  -> {'rows', 'shared', 'new', 'dropped_rows', 'dropped_points', 'saturated'}: rows of this map after the call,
        voxels both maps held, voxels only `other` held, rows / points the regrid dropped, ray counts that were clamped -- Python integers, one
        read-back of the counters per attempt.  An empty `other` changes nothing."""
        self._merge_args(other, pose, AccumulatedCloud)
        self._ensure()
        other._ensure()
        res = dict(rows=self._n, shared=0, new=0, dropped_rows=0, dropped_points=0, saturated=0)
        if other._n == 0:
            return res
        if pose is not None:
            other, host = other._regrid(pose, self.voxel_size, None)
            res['dropped_rows'], res['dropped_points'] = host[native.REGRID_DROPPED_ROWS], host[native.REGRID_DROPPED_POINTS]
            res['saturated'] = host[native.REGRID_SATURATED]
        sidecar = self._pierced is not None or other._pierced is not None
        counters = torch.empty((native.MERGE_COUNTERS,), dtype=torch.int64, device=self.device)

        def attempt(capacity):
            pierced_out = torch.zeros((capacity,), dtype=torch.int32, device=self.device) if sidecar else None
            native.accum_merge(self._cur, self._n, self._pierced, other._cur, other._n, other._pierced, other._dropped, self._alt, pierced_out, counters,
                               self._state)
            host = counters.tolist()                               # the one read-back of an attempt
            ok = host[native.MERGE_STATUS] == native.ACCUM_OK      # the entry point has one other status: the result needs more rows
            return native.ACCUM_OK if ok else native.ACCUM_TOO_SMALL, host[native.MERGE_NEEDED], (host, pierced_out)
        host, pierced_out = self._grow('accum_merge', attempt)[1]
        if sidecar:
            if self._pierce_counters is None:
                self._pierce_counters = other._pierce_counters.clone()
            elif other._pierce_counters is not None:
                self._pierce_counters = self._pierce_counters + other._pierce_counters
            self._pierced = pierced_out
        self._n = host[native.MERGE_NEEDED]
        self._dropped += other._dropped
        res.update(rows=self._n, shared=host[native.MERGE_SHARED], new=host[native.MERGE_NEW], saturated=res['saturated'] + host[native.MERGE_SATURATED])
        return res

    # ---- compare, select, difference ---------------------------------------------------------------------------------------------------
    def _filter_args(self, min_count, max_moving_fraction):
        min_count = int(min_count)
        if min_count < 1:
            raise ValueError('min_count must be at least 1, got %r' % min_count)
        _moving_fraction(max_moving_fraction)
        return min_count

    def compare(self, other, max_distance=None, min_count=1, max_moving_fraction=None):
        """What changed between this map and another, on the device, in both directions (include/pcacc.h C13).  Neither map is modified.
        Both maps on one grid (other.voxel_size == self.voxel_size, the same device; regrid() brings a map onto another grid); `other` may be this
        map.  max_distance in (0, voxel_size] (None = voxel_size); min_count, max_moving_fraction: ONE filter, extract's, for both maps.
        -> {'self': {...}, 'other': {...}, 'counters': {...}}.  Each side has one row per row of that map's extract(min_count, max_moving_fraction),
        in its order (normals() and components() align the same way), as device tensors:
        status [V] u8, a sum of native.COMPARE_* bits: HELD (the other map has this voxel), SAME (and its extract under the filter returns it), NEAR
        (a centroid the other's extract returns lies within max_distance of this row's float64 centroid, among the 3 x 3 x 3 voxels around it);
        same_row [V] i32: the voxel's row of the other's extract (-1 without SAME); row [V] i32, distance [V] f64: the nearest such centroid's row
        there and the distance to it (-1, +inf without NEAR; ties go to the lowest voxel; for max_distance <= 0.9 voxel_size it is the nearest of the
        whole map); pierced [V] i32: the other's see_through count of this voxel (0 without HELD or without one).  The rows are valid until the
        next add, prune or merge of the map they index.
        counters: per side {'rows', 'kept', 'same', 'held', 'near', 'only'}, Python integers -- the one read-back; `only` counts kept rows with
        neither SAME nor NEAR."""
        self._peer('compare', other, AccumulatedCloud)
        if other.voxel_size != self.voxel_size:
            raise ValueError('compare: voxel sizes %r and %r differ; regrid() one map onto the other\'s grid first' % (self.voxel_size, other.voxel_size))
        max_distance = _max_distance(max_distance, self.voxel_size)
        min_count = self._filter_args(min_count, max_moving_fraction)
        self._ensure()
        other._ensure()
        res = native.accum_compare(self._cur, self._n, self._pierced, other._cur, other._n, other._pierced, self.voxel_size, max_distance, min_count,
                                   max_moving_fraction)
        host = res['counters'].tolist()                            # the one read-back
        out = {'counters': {}}
        for side, key, at in (('self', 'a', 0), ('other', 'b', native.COMPARE_SIDE_COUNTERS)):
            c = dict(zip(_COMPARE_COUNTERS, host[at:at + native.COMPARE_SIDE_COUNTERS]))
            out[side] = {name: t[:c['kept']] for name, t in res[key].items()}
            out['counters'][side] = c
        return out

    def select(self, mask, invert=False, min_count=1, max_moving_fraction=None, capacity=None):
        """The rows of extract(min_count, max_moving_fraction) that mask [V] bool / uint8 (device) names -- with invert=True the rows it does not name
        -- as a NEW AccumulatedCloud on the same device (include/pcacc.h C13); this map is not modified.  Rows outside the filter are never
        selected.  Records, stamps and ray counts are copied bit for bit, the see_through counters are carried, `dropped` starts at 0.  capacity
        (None = this map's) must hold this map's rows.  Only the four counters are read back."""
        if mask is None:
            raise ValueError('select needs a mask over the rows of extract()')
        mask = _row_mask('select', mask)
        min_count = self._filter_args(min_count, max_moving_fraction)
        new = self._like(self.voxel_size, self._room(capacity))
        self._ensure()
        new._ensure()
        counters = torch.empty((native.SELECT_COUNTERS,), dtype=torch.int64, device=self.device)
        native.accum_select(self._cur, self._n, self._pierced, min_count, max_moving_fraction, mask, bool(invert), new._cur, new._pierced, counters,
                            new._state)
        host = counters.tolist()                                   # the one read-back of a select
        if host[native.SELECT_STATUS] == native.SELECT_BAD_MASK:
            raise _bad_mask(host[native.SELECT_KEPT])
        new._n = host[native.SELECT_SELECTED]
        return new

    def difference(self, other, max_distance=None, min_count=1, max_moving_fraction=None):
        """What this map has and `other` has nothing near: select() of the rows of extract(min_count, max_moving_fraction) that compare(other,
        max_distance, min_count, max_moving_fraction) gives neither SAME nor NEAR, as a NEW AccumulatedCloud."""
        status = self.compare(other, max_distance, min_count, max_moving_fraction)['self']['status']
        return self.select(~(status & (native.COMPARE_SAME | native.COMPARE_NEAR)).bool(), min_count=min_count, max_moving_fraction=max_moving_fraction)

    def save_ply(self, path, normals=True, min_count=1, max_moving_fraction=None, **normal_args):
        """extract(min_count, max_moving_fraction) as a binary PLY: x y z, with normals=True nx ny nz of normals(**normal_args) under the same filter
        (rows without a valid normal are kept, with a zero normal), then count, moving, t_first, t_last and, once see_through has run, pierced."""
        cloud = self.extract(min_count, max_moving_fraction)
        nrm = self.normals(min_count=min_count, max_moving_fraction=max_moving_fraction, **normal_args)['normals'] if normals else None
        fields = [(k, cloud[k]) for k in ('count', 'moving', 't_first', 't_last')]
        if self._pierced is not None:
            fields.append(('pierced', self.pierced(min_count, max_moving_fraction)))
        write_ply(path, cloud['points'], nrm, fields)

    # ---- persistence -------------------------------------------------------------------------------------------------------------------
    def records(self):
        """The integer records of the map as host arrays: keys [M] i64, acc [5,M] i64 (count, moving, sum q_x, sum q_y, sum q_z), stamps [2,M] i32."""
        return self._records()

    def save(self, path):
        keys, acc, stamps = self.records()
        extra = {}
        if self._pierced is not None:                              # a map that was never pierced saves what it always saved
            extra = {'pierced': self._pierced[:self._n].cpu().numpy(), 'pierce_counters': self._pierce_counters.cpu().numpy()}
        with open(path, 'wb') as f:
            np.savez(f, keys=keys, acc=acc, stamps=stamps, voxel_size=np.float64(self.voxel_size), dropped=np.int64(self._dropped), **extra)

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path, allow_pickle=False) as z:
            keys, acc, stamps = z['keys'], z['acc'], z['stamps']
            voxel_size, dropped = float(z['voxel_size']), int(z['dropped'])
            pierced = z['pierced'] if 'pierced' in z.files else None
            counters = z['pierce_counters'] if 'pierce_counters' in z.files else None
        m = keys.shape[0]
        if keys.dtype != np.int64 or acc.dtype != np.int64 or stamps.dtype != np.int32 or acc.shape != (native.ACCUM_FIELDS, m) or stamps.shape != (2, m):
            raise ValueError('%s does not hold the records of an AccumulatedCloud' % path)
        cls._ascending(path, keys)
        if (pierced is None) != (counters is None) or (pierced is not None and (pierced.dtype != np.int32 or pierced.shape != (m,) or counters.dtype != np.int64
                                                                                 or counters.shape != (native.PIERCE_COUNTERS,))):
            raise ValueError('%s does not hold the ray counts of an AccumulatedCloud' % path)
        self = cls._from_records((keys, acc, stamps), voxel_size, device)
        host = [0] * native.ACCUM_STATE_WORDS
        host[native.ACCUM_NUM_VOXELS], host[native.ACCUM_DROPPED] = m, dropped
        self._state.copy_(torch.tensor(host, dtype=torch.int64))
        self._dropped = dropped
        if pierced is not None:
            self._pierced = torch.zeros((self.capacity,), dtype=torch.int32, device=self.device)
            self._pierced[:m] = torch.from_numpy(pierced).to(self.device)
            self._pierce_counters = torch.from_numpy(counters).to(self.device)
        return self


def _observe_chunks(n, max_steps):
    """[(lo, hi)]: the rays 0..n cut into runs with (hi - lo) * max_steps < 2^31, the most visits the int32 offsets of one call hold."""
    per_call = (native.OBSERVE_MAX_VISITS - 1) // int(max_steps)
    return [(lo, min(lo + per_call, n)) for lo in range(0, n, per_call)]


def _observed_tables(capacity, device):
    return (torch.empty((capacity,), dtype=torch.int64, device=device), torch.empty((capacity,), dtype=torch.int64, device=device),
            torch.empty((2, capacity), dtype=torch.int32, device=device))


_OBSERVE_COUNTERS = ('walked', 'dropped', 'skipped', 'truncated', 'visits')
UNKNOWN, FREE, OCCUPIED = 0, 1, 2                                  # occupancy()'s three states


class ObservedSpace(_VoxelTable):
    """Where the sensor looked and found nothing: the voxels that measured rays crossed, as a second sorted table on the device (include/pcacc.h C14,
    DESIGN.md section 9n).  Per voxel the number of rays that crossed it and the first / last stamp of the calls in which one did.  With an
    AccumulatedCloud on the same grid a voxel is OCCUPIED, FREE or UNKNOWN (occupancy()); its own lookup() works at any voxel size, so free space may
    be kept coarser than the cloud.  All integers: the table is a function of the set of (ray, stamp) pairs it was given.  No CPU path."""

    _tables, _state_words, _noun = staticmethod(_observed_tables), native.OBSERVE_STATE_WORDS, 'table'

    def __init__(self, voxel_size, device='cuda', capacity=1 << 20, visit_budget=1 << 26):
        super(ObservedSpace, self).__init__(voxel_size, device, capacity)
        if not 1 <= int(visit_budget) < native.OBSERVE_MAX_VISITS:
            raise ValueError('visit_budget must lie in [1, 2^31), got %r' % visit_budget)
        self.visit_budget = int(visit_budget)
        self._counters = [0] * len(_OBSERVE_COUNTERS)
        self.splits = 0                                      # times a call's rays had to be cut for the visit budget, since clear()
        self.dropped_rows = 0                                # of a table that regrid() made: the rows that left the grid under the pose

    # ---- state -------------------------------------------------------------------------------------------------------------------------
    @property
    def counters(self):
        """{'walked', 'dropped', 'skipped', 'truncated', 'visits'}: rays and visited voxels of every observe since clear(), Python integers."""
        return dict(zip(_OBSERVE_COUNTERS, self._counters))

    def _write_state(self):
        host = [0] * native.OBSERVE_STATE_WORDS
        host[native.OBSERVE_NUM_VOXELS] = self._n
        host[native.OBSERVE_WALKED:native.OBSERVE_WALKED + len(_OBSERVE_COUNTERS)] = self._counters
        self._state.copy_(torch.tensor(host, dtype=torch.int64))

    def clear(self):
        self._n = 0
        self._counters = [0] * len(_OBSERVE_COUNTERS)
        self.splits = 0
        if self._state is not None:
            self._state.zero_()

    # ---- observe -----------------------------------------------------------------------------------------------------------------------
    def observe(self, points, origins, origin_index=None, pose=None, moving=None, stamp=0, margin=None, max_range=None, max_steps=4096):
        """Record the voxels the measured rays of a scan cross (include/pcacc.h C14).  The arguments are see_through()'s and a ray is its ray, bit for
        bit: points [n,3] f32 (device, scan frame); origins [3] or [S,3]; origin_index [n] integers (device; None = row 0); pose [4,4] scan-to-world;
        moving [n] (non-zero: the ray is skipped); margin (None = 2 voxel_size): the ray stops this far in front of the point it measured; max_range;
        max_steps in [1, 2^16].  stamp: one integer for the call.  Every voxel a walked ray visits, its start voxel included, gains one ray and takes
        the stamp into its first / last.
        The rays are cut into calls of fewer than 2^31 possible visits; a call whose rays make more than visit_budget visits is cut again.  The table
        grows by doubling as add() does.  One read-back of the state words per attempt.  -> self."""
        n = _scan_points('observe', 'points', points, native.ACCUM_MAX_POINTS)
        _scan_rows('observe', 'moving', moving, n)
        _scan_rows('observe', 'origin_index', origin_index, n)
        origins = _origins(origins)
        margin = 2.0 * self.voxel_size if margin is None else float(margin)
        _margin(margin)
        _max_range(max_range)
        max_steps = int(max_steps)
        _max_steps(max_steps, native.PIERCE_MAX_STEPS)
        if self.visit_budget < max_steps:
            raise ValueError('visit_budget %d is below max_steps %d: a single ray must fit' % (self.visit_budget, max_steps))
        _stamp32('stamp', stamp)
        pose = self._pose(pose)
        if n == 0:
            return self
        self._ensure()
        pts = points.detach().float().contiguous()
        mv = (moving != 0).to(torch.uint8).contiguous() if moving is not None else None
        idx = _origin_rows(origin_index, origins.shape[0])
        org = origins.to(device=self.device, dtype=torch.float64).contiguous()
        work = _observe_chunks(n, max_steps)[::-1]                 # a stack: the next rays on top
        while work:
            lo, hi = work.pop()
            needed = self._observe_rows(pts[lo:hi], None if mv is None else mv[lo:hi], org, None if idx is None else idx[lo:hi], pose, int(stamp), margin,
                                        max_range, max_steps)
            if needed:                                             # more visits than the budget: cut these rays and go on
                pieces = min(-(-needed // self.visit_budget), hi - lo)
                if pieces < 2:
                    raise native.NativeError('accum_observe: %d rays make %d visits, which a budget of %d must hold' % (hi - lo, needed, self.visit_budget))
                self.splits += 1
                cuts = [lo + (hi - lo) * k // pieces for k in range(pieces + 1)]
                work.extend((a, b) for a, b in list(zip(cuts[:-1], cuts[1:]))[::-1] if b > a)
        return self

    def _observe_rows(self, pts, mv, org, idx, pose, stamp, margin, max_range, max_steps):
        """One run of rays through the double-the-tables loop of add().  -> 0, or the visits of a run that exceeds the budget (nothing has changed)."""
        visit_capacity = min(self.visit_budget, pts.shape[0] * max_steps)

        def attempt(capacity):
            native.accum_observe(pts, mv, org, idx, pose, stamp, self.voxel_size, margin, max_range, max_steps, visit_capacity, self._cur, self._n, self._alt,
                                 self._state)
            state = self._state.tolist()                           # the one read-back of an attempt
            return state[native.OBSERVE_STATUS], state[native.OBSERVE_NEEDED], state
        status, state = self._grow('accum_observe', attempt, leave=(native.OBSERVE_TOO_MANY,))
        if status == native.OBSERVE_TOO_MANY:
            return state[native.OBSERVE_NEEDED_VISITS]
        self._n = state[native.OBSERVE_NUM_VOXELS]
        self._counters = state[native.OBSERVE_WALKED:native.OBSERVE_WALKED + len(_OBSERVE_COUNTERS)]
        return 0

    def observe_results(self, results, input_dict, pose=None, sensor_offset=(0, 0, 0), stamp=0, **kw):
        """observe() of a test / val-mode forward, with the rays see_through_results builds: the points are results['rec_est'] with
        results['mos_est'].argmax(1) == 1 as `moving`, the origin of a point is the sensor position of its frame in the anchor frame.  One sample per
        batch."""
        _one_sample(results, input_dict, 'observe_results')
        return self.observe(results['rec_est'], _sensor_origins(results, sensor_offset), input_dict['time_indice'][:, 1], pose,
                            results['mos_est'].argmax(1) == 1, stamp, **kw)

    # ---- read --------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _min_rays(min_rays):
        min_rays = int(min_rays)
        if min_rays < 1:
            raise ValueError('min_rays must be at least 1, got %r' % min_rays)
        return min_rays

    def extract(self, min_rays=1):
        """One row per voxel that at least min_rays rays crossed, in ascending (x, y, z) voxel order: coords [V,3] i32, centers [V,3] f32 (the middle
        of the voxel), rays [V] i64, t_first, t_last [V] i32."""
        min_rays = self._min_rays(min_rays)
        self._ensure()
        keys, rays, stamps = (t[..., :self._n] for t in self._cur)
        keep = rays >= min_rays
        coords = _voxel_coords(keys[keep])
        centers = ((coords.to(torch.float64) + 0.5) * self.voxel_size).to(torch.float32)
        return {'coords': coords.to(torch.int32), 'centers': centers, 'rays': rays[keep], 't_first': stamps[0][keep], 't_last': stamps[1][keep]}

    def lookup(self, points, pose=None, min_rays=1):
        """What the table knows at every point of a scan: points [n,3] f32 (device), pose [4,4] scan-to-world (None = identity).
        -> dict of device tensors, one row per point: status [n] u8, a sum of native.OBSERVED_VALID (the point is finite and inside the grid),
        OBSERVED_SEEN (a ray crossed its voxel), OBSERVED_ENOUGH (at least min_rays did); rays [n] i64, t_first, t_last [n] i32 (0 where unseen);
        counters [4] i64: rows, valid, seen, enough.  Nothing is read back."""
        _scan_points('lookup', 'points', points, native.ACCUM_MAX_POINTS)
        min_rays = self._min_rays(min_rays)
        pose = self._pose(pose)
        self._ensure()
        return native.accum_observed_lookup(points.detach().float().contiguous(), None, pose, self.voxel_size, self._cur, self._n, min_rays)

    def lookup_voxels(self, coords, min_rays=1):
        """lookup() of voxel index rows: coords [n,3] integers (device), e.g. extract()['coords'] of a cloud on the same grid.  A row with an index
        outside [-2^20, 2^20) is not VALID."""
        _scan_points('lookup_voxels', 'coords', coords, native.ACCUM_MAX_POINTS, 'rows')
        if coords.dtype not in (torch.int32, torch.int64):
            raise ValueError('coords must be int32 or int64 voxel indices, got %s' % coords.dtype)
        min_rays = self._min_rays(min_rays)
        self._ensure()
        if coords.dtype == torch.int64:                            # an index outside the grid stays outside after the cast
            coords = coords.clamp(-native.ACCUM_IDX_BIAS - 1, native.ACCUM_IDX_BIAS)
        return native.accum_observed_lookup(None, coords.to(torch.int32).contiguous(), None, self.voxel_size, self._cur, self._n, min_rays)

    def occupancy(self, cloud, coords, min_count=1, max_moving_fraction=None, min_rays=1):
        """The state of every voxel index row of coords [n,3] -> [n] uint8: OCCUPIED (2) where cloud.extract(min_count, max_moving_fraction) holds the
        voxel, else FREE (1) where at least min_rays rays crossed it, else UNKNOWN (0).  A key join, as AccumulatedCloud.pierced() is; cloud and
        table on one grid and one device."""
        if not isinstance(cloud, AccumulatedCloud):
            raise TypeError('occupancy takes an AccumulatedCloud, got %s' % type(cloud).__name__)
        if cloud.voxel_size != self.voxel_size:
            raise ValueError('occupancy: voxel sizes %r and %r differ' % (self.voxel_size, cloud.voxel_size))
        if _device_key(cloud.device) != _device_key(self.device):
            raise ValueError('occupancy: the cloud lives on %s and the table on %s' % (cloud.device, self.device))
        seen = self.lookup_voxels(coords, min_rays)['status']
        out = ((seen & native.OBSERVED_ENOUGH) != 0).to(torch.uint8) * FREE
        held = _voxel_keys(cloud.extract(min_count, max_moving_fraction)['coords'])       # ascending: extract is in key order
        valid = (seen & native.OBSERVED_VALID) != 0
        if held.shape[0] and coords.shape[0]:
            keys = torch.where(valid, _voxel_keys(coords.clamp(-native.ACCUM_IDX_BIAS, native.ACCUM_IDX_BIAS - 1)), torch.full_like(held[:1], -1))
            at = torch.searchsorted(held, keys).clamp(max=held.shape[0] - 1)
            out[(held[at] == keys) & valid] = OCCUPIED
        return out

    # ---- forget ------------------------------------------------------------------------------------------------------------------------
    def forget(self, before_stamp=None, box=None):
        """Rows leave the table: those whose last stamp is below before_stamp and those whose voxel lies outside box = (lo [3], hi [3]), metres, both
        faces' voxels included (prune()'s rule).  The order of the rows that stay is preserved.  -> the number kept."""
        if before_stamp is not None:
            _stamp32('before_stamp', before_stamp)
        if box is not None:
            box = self._box_indices(box)
        self._ensure()
        n = self._n
        keys, rays, stamps = self._cur
        keep = torch.ones((n,), dtype=torch.bool, device=self.device)
        if before_stamp is not None:
            keep &= stamps[1, :n] >= int(before_stamp)
        if box is not None:
            coords = _voxel_coords(keys[:n])
            for axis, (lo, hi) in enumerate(zip(*box)):
                keep &= (coords[:, axis] >= lo) & (coords[:, axis] <= hi)
        kept = int(keep.sum())                                     # the one read-back
        if kept != n:
            keys[:kept], rays[:kept] = keys[:n][keep], rays[:n][keep]
            stamps[:, :kept] = stamps[:, :n][:, keep]
            self._n = kept
            self._write_state()
        return kept

    # ---- copy, regrid, merge -----------------------------------------------------------------------------------------------------------
    def copy(self):
        """An independent clone: device copies of the rows in use and of the state words, the counters and visit_budget; its `splits` start at 0.
        merge() mutates its space, so `c = a.copy(); c.merge(b)` keeps a."""
        c = self._copy_rows(ObservedSpace(self.voxel_size, self.device, self.capacity, self.visit_budget))
        c._counters = list(self._counters)
        return c

    def _regrid(self, pose, voxel_size, capacity):
        voxel_size, capacity = self._regrid_args(pose, voxel_size, capacity)
        new = ObservedSpace(voxel_size, self.device, capacity, self.visit_budget)      # checks voxel_size and capacity
        pose = self._pose(pose)
        self._ensure()
        new._ensure()
        counters = torch.empty((native.OBSERVED_REGRID_COUNTERS,), dtype=torch.int64, device=self.device)
        native.accum_observed_regrid(self._cur, self._n, self._state, pose, self.voxel_size, voxel_size, new._cur, counters, new._state)
        host = counters.tolist()                                   # the one read-back of a regrid
        if host[native.OBSERVED_REGRID_ROWS_IN] != self._n:
            raise native.NativeError('accum_observed_regrid: the state words do not describe the table')
        new._n = host[native.OBSERVED_REGRID_ROWS_OUT]
        new._counters = list(self._counters)
        new.dropped_rows = host[native.OBSERVED_REGRID_DROPPED_ROWS]
        return new

    def regrid(self, pose=None, voxel_size=None, capacity=None):
        """This table under a rigid pose ([4,4] table-to-new-frame, tensor or array) and / or at another voxel size, as a NEW ObservedSpace on the same
        device (include/pcacc.h C15); this one is not modified.  LOSSY by declared contract: a row is treated as the centre of its voxel.  Rows that
        land in one new voxel become one row with the MAXIMUM of their ray counts (a ray that crossed several of them is one ray: the sum would
        overstate the evidence for "free"), the minimum first and the maximum last stamp.  A row whose centre leaves the grid (or is not finite
        under the pose) is dropped, never clamped; the result's attribute `dropped_rows` says how many.  The counters are carried over: they
        describe the rays, and `visits` no longer equals the sum of `rays`.  Identity and the same voxel size return the same table; an integer
        multiple of the voxel size is an exact coarsening.  With a rotation pick a COARSER voxel_size (twice this one): at the same size a
        rotated grid leaves holes -- in one sample of a 30 degree turn about z, 13.4 % of the destination voxels received no centre, at twice the
        size none -- and a hole reads UNKNOWN.  capacity (None = this one's) must hold this table's rows.  Only the three counters are read back."""
        return self._regrid(pose, voxel_size, capacity)

    def merge(self, other, pose=None):
        """Take another table's voxels into this one, on the device (include/pcacc.h C15); `other` is not modified.
        pose=None is the exact path: both tables on one grid (other.voxel_size == self.voxel_size, the same device), and the result is, integer for
        integer, the table and the counters one ObservedSpace would hold had it been given every observe of both: ray counts added, first stamp the
        minimum, last stamp the maximum.  With a pose ([4,4] other-to-world, tensor or array) `other` is first regridded under it onto this table's
        voxel size (regrid: lossy by declared contract) and the result merged.
        The capacity grows as in observe().  -> {'rows', 'shared', 'new', 'dropped_rows'}: rows of this table after the call, voxels both held,
        voxels only `other` held, rows the regrid dropped -- Python integers, one read-back of the counters per attempt.  An empty `other` changes
        nothing."""
        self._merge_args(other, pose, ObservedSpace)
        pose = self._pose(pose)
        self._ensure()
        other._ensure()
        res = dict(rows=self._n, shared=0, new=0, dropped_rows=0)
        if other._n == 0:
            return res
        if pose is not None:
            other = other._regrid(pose, self.voxel_size, None)
            res['dropped_rows'] = other.dropped_rows
        counters = torch.empty((native.OBSERVED_MERGE_COUNTERS,), dtype=torch.int64, device=self.device)

        def attempt(capacity):
            native.accum_observed_merge(self._cur, self._n, other._cur, other._n, other._state, self._alt, counters, self._state)
            host = counters.tolist()                               # the one read-back of an attempt
            return host[native.OBSERVED_MERGE_STATUS], host[native.OBSERVED_MERGE_NEEDED], host
        host = self._grow('accum_observed_merge', attempt, described='tables')[1]
        self._n = host[native.OBSERVED_MERGE_NEEDED]
        self._counters = [a + b for a, b in zip(self._counters, other._counters)]
        res.update(rows=self._n, shared=host[native.OBSERVED_MERGE_SHARED], new=host[native.OBSERVED_MERGE_NEW])
        return res

    # ---- persistence -------------------------------------------------------------------------------------------------------------------
    def records(self):
        """The integer columns as host arrays: keys [M] i64, rays [M] i64, stamps [2,M] i32."""
        return self._records()

    def save(self, path):
        keys, rays, stamps = self.records()
        with open(path, 'wb') as f:
            np.savez(f, keys=keys, rays=rays, stamps=stamps, counters=np.array(self._counters, np.int64), voxel_size=np.float64(self.voxel_size))

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path, allow_pickle=False) as z:
            keys, rays, stamps, counters, voxel_size = z['keys'], z['rays'], z['stamps'], z['counters'], float(z['voxel_size'])
        m = keys.shape[0]
        if keys.dtype != np.int64 or rays.dtype != np.int64 or stamps.dtype != np.int32 or counters.dtype != np.int64 or keys.ndim != 1 \
                or rays.shape != (m,) or stamps.shape != (2, m) or counters.shape != (len(_OBSERVE_COUNTERS),):
            raise ValueError('%s does not hold the columns of an ObservedSpace' % path)
        cls._ascending(path, keys)
        self = cls._from_records((keys, rays, stamps), voxel_size, device)
        self._counters = [int(v) for v in counters]
        self._write_state()
        return self


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_ply(path, points, normals=None, fields=None):
    """A binary little-endian PLY of V vertices from host or device arrays: x y z (float), nx ny nz (float) when normals [V,3] is given, then one
    scalar property per entry of fields -- a dict or a list of (name, [V] array) -- in its order and in the array's own type (64-bit integers, which
    PLY does not have, as int; values outside int32 raise ValueError)."""
    pts = np.ascontiguousarray(_host(points), dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError('points must be [V,3], got %s' % (pts.shape,))
    v = pts.shape[0]
    cols = [(n, pts[:, a]) for a, n in enumerate(('x', 'y', 'z'))]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals), dtype=np.float32)
        if nrm.shape != (v, 3):
            raise ValueError('normals must be [%d,3], got %s' % (v, nrm.shape))
        cols += [(n, nrm[:, a]) for a, n in enumerate(('nx', 'ny', 'nz'))]
    for name, col in (fields.items() if isinstance(fields, dict) else (fields or ())):
        col = _host(col)
        if col.dtype == np.bool_:
            col = col.astype(np.uint8)
        if col.dtype in (np.int64, np.uint64):
            if v and (col.max() > np.iinfo(np.int32).max or col.min() < np.iinfo(np.int32).min):
                raise ValueError('write_ply: %s does not fit the 32-bit integer of a PLY property' % name)
            col = col.astype(np.int32)
        if col.shape != (v,) or col.dtype.name not in _PLY_TYPES:
            raise ValueError('write_ply: %s must be a [%d] column of a PLY scalar type, got %s %s' % (name, v, col.shape, col.dtype))
        if not str(name).isidentifier() or name in [c[0] for c in cols]:
            raise ValueError('write_ply: %r is no new property name' % (name,))
        cols.append((str(name), col))
    rows = np.empty((v,), dtype=[(n, c.dtype.newbyteorder('<')) for n, c in cols])
    for n, c in cols:
        rows[n] = c
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % v]
    header += ['property %s %s' % (_PLY_TYPES[c.dtype.name], n) for n, c in cols]
    with open(path, 'wb') as f:
        f.write(('\n'.join(header + ['end_header']) + '\n').encode('ascii'))
        f.write(rows.tobytes())


def voxel_mean_downsample(points, voxel_size):
    """One centroid per occupied voxel of `points` [n,3] (device), in ascending (x, y, z) voxel order: one add and one extract."""
    n = points.shape[0] if torch.is_tensor(points) and points.dim() == 2 else 0
    capacity = 64
    while capacity < n:
        capacity *= 2
    return AccumulatedCloud(voxel_size, points.device if torch.is_tensor(points) else 'cuda', capacity).add(points).extract()['points']
