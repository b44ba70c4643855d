"""The host classes of the accumulated cloud, pcaccumulation_amd/accumulate.py: AccumulatedCloud and ObservedSpace on their
shared base, held to what they did before they had one.

Error table: every argument check that fires with no tensor or with a CPU tensor (CPU leg) and those that need a tensor on the GPU (GPU leg), each
with its exception type and its full message.
Call transcript: one scripted session through every method of both classes with every native.accum_* entry point replaced by a recorder; the calls
and their arguments, the integer dicts the methods return and the records of every map and table at the end equal
tests/golden/accum_host_transcript.json, which `python tests/test_accumulate_host.py --record` writes (on a GPU).
Structure: each mechanism the two classes share stands once in the text of accumulate.py."""
import hashlib
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import accumulate_helpers as ah                                                 # noqa: E402
from accumulate_helpers import DEV                                              # noqa: E402
from pcaccumulation_amd import accumulate, native                               # noqa: E402
from pcaccumulation_amd.accumulate import AccumulatedCloud, ObservedSpace       # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'accum_host_transcript.json')
RECORDED_AT = '46055f8'                                                          # the commit whose accumulate.py the golden file was recorded from
RECORDED_FROM = 'b2592cdde8b6e0e7f7f91ccb186dc94a67c7af8f8ccc6cf006f0fd2d12e17243'      # sha256 of that file: --record runs on no other text

NO_CPU = '; the HIP path has no CPU fallback'
ON_GPU = ' must be a tensor on the GPU' + NO_CPU
CLOUD_CPU = 'AccumulatedCloud lives on the GPU (got device cpu)' + NO_CPU
SPACE_CPU = 'ObservedSpace lives on the GPU (got device cpu)' + NO_CPU
MASK = 'mask must be a 1-D bool / uint8 tensor over the rows of extract()'
MMF = 'max_moving_fraction must be a number or None'
BOX = 'box must be (lo [3], hi [3]) in metres, got '
FIELD_CELLS = ' cells: at most 2^28; give a smaller box, a smaller max_radius or pad=False'
VOXEL_SIZES = 'voxel sizes 0.1 and 0.2 differ'
CARRIES = '; save() / load() carries a map across'

# (expression, exception, message).  C / S: a cloud / a space of voxel size 0.1 and capacity 64 that has taken no device memory; C2 / S2: the same at
# 0.2; Ccpu / Scpu: on the device 'cpu'.  P [4,3] f32, I [4,3] i32, B [3] bool, F [3] f32: tensors (on the CPU in the CPU table, on the GPU in the
# other); R2, D: a forward's results that say they hold two samples, and its input_dict; FIELD: what inflate() reads of a distance_field().
CPU_CASES = [
    # ---- the constructors
    ('AccumulatedCloud(0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('AccumulatedCloud(inf)', ValueError, 'voxel_size must be a positive finite number, got inf'),
    ('AccumulatedCloud(nan)', ValueError, 'voxel_size must be a positive finite number, got nan'),
    ('AccumulatedCloud(0.1, "cuda", 0)', ValueError, 'capacity must lie in [1, 2^30], got 0'),
    ('AccumulatedCloud(0.1, "cuda", (1 << 30) + 1)', ValueError, 'capacity must lie in [1, 2^30], got 1073741825'),
    ('AccumulatedCloud(0, "cuda", 0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('ObservedSpace(0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('ObservedSpace(nan)', ValueError, 'voxel_size must be a positive finite number, got nan'),
    ('ObservedSpace(0.1, "cuda", 0)', ValueError, 'capacity must lie in [1, 2^30], got 0'),
    ('ObservedSpace(0.1, "cuda", (1 << 30) + 1)', ValueError, 'capacity must lie in [1, 2^30], got 1073741825'),
    ('ObservedSpace(0.1, visit_budget=0)', ValueError, 'visit_budget must lie in [1, 2^31), got 0'),
    ('ObservedSpace(0.1, visit_budget=1 << 31)', ValueError, 'visit_budget must lie in [1, 2^31), got 2147483648'),
    ('ObservedSpace(0.1, "cuda", 0, 0)', ValueError, 'capacity must lie in [1, 2^30], got 0'),
    # ---- the device and the pose
    ('Ccpu.extract()', native.NativeError, CLOUD_CPU),
    ('Scpu.extract()', native.NativeError, SPACE_CPU),
    ('C._pose(np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('C._pose(torch.zeros(4))', ValueError, 'pose must be [4,4], got (4,)'),
    ('S._pose(np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    # ---- the scans: a CPU tensor is refused before any other argument is looked at
    ('C.add(None)', native.NativeError, 'add: points' + ON_GPU),
    ('C.add(P, np.eye(3))', native.NativeError, 'add: points' + ON_GPU),
    ('C.register(P, max_distance=0)', native.NativeError, 'register: points' + ON_GPU),
    ('C.query(P, radius=4)', native.NativeError, 'query: points' + ON_GPU),
    ('C.knn(P, 0)', native.NativeError, 'knn: points' + ON_GPU),
    ('C.see_through(P, np.zeros(2), margin=-1)', native.NativeError, 'see_through: points' + ON_GPU),
    ('C.raycast(P, np.zeros(2), max_steps=0)', native.NativeError, 'raycast: targets' + ON_GPU),
    ('C.clearance(points=P)', native.NativeError, 'clearance: points' + ON_GPU),
    ('C.clearance(coords=I)', native.NativeError, 'clearance: coords' + ON_GPU),
    ('S.observe(P, np.zeros(2), stamp=1 << 31)', native.NativeError, 'observe: points' + ON_GPU),
    ('S.lookup(P, min_rays=0)', native.NativeError, 'lookup: points' + ON_GPU),
    ('S.lookup_voxels(I, min_rays=0)', native.NativeError, 'lookup_voxels: coords' + ON_GPU),
    ('C.add_results(R2, D)', ValueError, 'add_results: 2 samples in the batch need one pose per sample, [B,4,4]'),
    ('C.register_results(R2, D)', ValueError, 'register_results: one sample per batch, got 2'),
    ('C.query_results(R2, D)', ValueError, 'query_results: one sample per batch, got 2'),
    ('C.knn_results(R2, D)', ValueError, 'knn_results: one sample per batch, got 2'),
    ('C.see_through_results(R2, D)', ValueError, 'see_through_results: one sample per batch, got 2'),
    ('C.raycast_results(R2, D)', ValueError, 'raycast_results: one sample per batch, got 2'),
    ('S.observe_results(R2, D)', ValueError, 'observe_results: one sample per batch, got 2'),
    # ---- normals
    ('C.normals(radius=4)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.normals(radius=0, min_neighbors=2)', ValueError, 'radius must be 1, 2 or 3 voxels, got 0'),
    ('C.normals(min_neighbors=2)', ValueError, 'min_neighbors must be at least 3, got 2'),
    ('C.normals(min_neighbors=2, viewpoints=np.zeros(3))', ValueError, 'min_neighbors must be at least 3, got 2'),
    ('C.normals(viewpoints=np.zeros(3))', ValueError, 'viewpoints must be [S,3], got (3,)'),
    ('C.normals(viewpoints=torch.zeros(2, 2))', ValueError, 'viewpoints must be [S,3], got (2, 2)'),
    ('Ccpu.normals(min_count=0)', native.NativeError, CLOUD_CPU),
    # ---- k nearest
    ('C.neighbors(0)', ValueError, 'k must lie in [1, 16], got 0'),
    ('C.neighbors(17, radius=0)', ValueError, 'k must lie in [1, 16], got 17'),
    ('C.neighbors(4, radius=0)', ValueError, 'radius must lie in [1, 4] voxels, got 0'),
    ('C.neighbors(4, radius=5, max_distance=0)', ValueError, 'radius must lie in [1, 4] voxels, got 5'),
    ('C.neighbors(4, max_distance=0)', ValueError, 'max_distance must lie in (0, radius * voxel_size = 0.2], got 0.0'),
    ('C.neighbors(4, radius=1, max_distance=0.2)', ValueError, 'max_distance must lie in (0, radius * voxel_size = 0.1], got 0.2'),
    ('Ccpu.neighbors(4, min_count=0)', native.NativeError, CLOUD_CPU),
    ('C.outliers(std_ratio=inf)', ValueError, 'std_ratio must be finite, got inf'),
    ('C.outliers(std_ratio=nan, k=0)', ValueError, 'std_ratio must be finite, got nan'),
    ('C.outliers(k=0)', ValueError, 'k must lie in [1, 16], got 0'),
    # ---- columns, ground, bird's-eye view
    ('C.columns(ground_radius=-1)', ValueError, 'ground_radius must lie in [0, 8] columns, got -1'),
    ('C.columns(ground_radius=9, thickness=-1)', ValueError, 'ground_radius must lie in [0, 8] columns, got 9'),
    ('C.columns(thickness=-1, band=None)', ValueError, 'thickness must lie in [0, 2^21) voxels, got -1'),
    ('C.columns(thickness=1 << 21)', ValueError, 'thickness must lie in [0, 2^21) voxels, got 2097152'),
    ('C.columns(band=None)', ValueError, 'band must be (lo, hi) in voxels above the ground, got None'),
    ('C.columns(band=(1,))', ValueError, 'band must be (lo, hi) in voxels above the ground, got (1,)'),
    ('C.columns(band=(3, 1), min_count=0)', ValueError, 'band must hold 0 <= lo <= hi < 2^21, got (3, 1)'),
    ('C.columns(band=(-1, 1))', ValueError, 'band must hold 0 <= lo <= hi < 2^21, got (-1, 1)'),
    ('C.columns(band=(0, 1 << 21))', ValueError, 'band must hold 0 <= lo <= hi < 2^21, got (0, 2097152)'),
    ('C.columns(min_count=0, max_moving_fraction=nan)', ValueError, 'min_count must be at least 1, got 0'),
    ('C.columns(max_moving_fraction=nan)', ValueError, MMF),
    ('Ccpu.columns()', native.NativeError, CLOUD_CPU),
    ('C.ground_mask(band=(3, 1))', ValueError, 'band must hold 0 <= lo <= hi < 2^21, got (3, 1)'),
    ('C.split_ground(min_count=0)', ValueError, 'min_count must be at least 1, got 0'),
    ('C.bev(origin=(1,))', ValueError, 'origin must be (x0, y0) in voxel indices, got (1,)'),
    ('C.bev(origin=((1 << 31) + 1, 0), shape=(0, 1))', ValueError, 'origin must be (x0, y0) in voxel indices, got (2147483649, 0)'),
    ('C.bev(shape=(1,))', ValueError, 'shape must be (H, W) with H, W >= 1 and at most 2^28 pixels, got (1,)'),
    ('C.bev(shape=(0, 1), band=None)', ValueError, 'shape must be (H, W) with H, W >= 1 and at most 2^28 pixels, got (0, 1)'),
    ('C.bev(shape=(1 << 14, 1 << 15))', ValueError, 'shape must be (H, W) with H, W >= 1 and at most 2^28 pixels, got (16384, 32768)'),
    ('C.bev(band=(3, 1))', ValueError, 'band must hold 0 <= lo <= hi < 2^21, got (3, 1)'),
    ('Ccpu.bev(origin=(0, 0), shape=(2, 2))', native.NativeError, CLOUD_CPU),
    # ---- distance field, clearance, inflation
    ('C.distance_field(max_radius=0)', ValueError, 'max_radius must lie in [1, 128] voxels, got 0'),
    ('C.distance_field(max_radius=129, origin=(0, 0))', ValueError, 'max_radius must lie in [1, 128] voxels, got 129'),
    ('C.distance_field(origin=(0, 0), shape=(0, 1, 1))', ValueError, 'origin must be (x0, y0, z0) in voxel indices, each at most 2^31 in size, got (0, 0)'),
    ('C.distance_field(origin=((1 << 31) + 1, 0, 0))', ValueError,
     'origin must be (x0, y0, z0) in voxel indices, each at most 2^31 in size, got (2147483649, 0, 0)'),
    ('C.distance_field(shape=(0, 1, 1), min_count=0)', ValueError, 'shape must be (nx, ny, nz) with every side >= 1, got (0, 1, 1)'),
    ('C.distance_field(shape=(1, 1))', ValueError, 'shape must be (nx, ny, nz) with every side >= 1, got (1, 1)'),
    ('C.distance_field(origin=(-(1 << 31), 0, 0), shape=(1, 1, 1), max_radius=1)', ValueError,
     'the box grown by max_radius starts at (-2147483649, -1, -1): beyond 2^31'),
    ('C.distance_field(origin=(-(1 << 31), 0, 0), shape=(1, 1, 1), max_radius=1, planar=True)', ValueError,
     'the box grown by max_radius starts at (-2147483649, -1, 0): beyond 2^31'),
    ('C.distance_field(origin=(0, 0, 0), shape=(1024, 1024, 1024), pad=False, min_count=0)', ValueError, 'the box has (1024, 1024, 1024)' + FIELD_CELLS),
    ('C.distance_field(origin=(0, 0, 0), shape=(1024, 1024, 1024))', ValueError, 'the box grown by max_radius has (1088, 1088, 1088)' + FIELD_CELLS),
    ('C.distance_field(min_count=0)', ValueError, 'min_count must be at least 1, got 0'),
    ('C.distance_field(max_moving_fraction=nan)', ValueError, MMF),
    ('Ccpu.distance_field()', native.NativeError, CLOUD_CPU),
    ('C.clearance()', ValueError, 'clearance: exactly one of points and coords'),
    ('C.clearance(P, I)', ValueError, 'clearance: exactly one of points and coords'),
    ('C.inflate(-1)', ValueError, 'radius_m must be a finite number >= 0, got -1.0'),
    ('C.inflate(nan, max_radius=0)', ValueError, 'radius_m must be a finite number >= 0, got nan'),
    ('C.inflate(1.0, max_radius=0)', ValueError, 'max_radius must lie in [1, 128] voxels, got 0'),
    ('C.inflate(1.0, field=FIELD, planar=True, pad=False)', ValueError, "inflate: a field and arguments for a new one: ['pad', 'planar']"),
    ('C.inflate(1.0, field=FIELD)', ValueError, 'radius_m is 10 voxels: above the max_radius 1 of the field'),
    # ---- raycast
    ('C.render_range_image(None, 0, 4, 0.1, -0.1, 5.0)', ValueError, 'height and width must be at least 1 and height * width at most 2^30, got 0 x 4'),
    ('C.render_range_image(None, 2, 4, nan, -0.1, None)', ValueError, 'fov_up and fov_down must be finite, got nan -0.1'),
    ('C.render_range_image(None, 2, 4, 0.1, -0.1, None)', ValueError, 'render_range_image needs a max_range: a direction has no target to stop at'),
    ('Ccpu.render_range_image(None, 2, 4, 0.1, -0.1, 5.0)', native.NativeError, 'raycast: targets' + ON_GPU),
    ('Ccpu.pierced()', native.NativeError, CLOUD_CPU),
    ('Ccpu.save_ply("no.ply")', native.NativeError, CLOUD_CPU),
    # ---- prune, forget
    ('C.prune(min_pierced=-1)', ValueError, 'min_pierced must be None or lie in [0, 2^31), got -1'),
    ('C.prune(min_pierced=1 << 31, pierced_ratio=-1)', ValueError, 'min_pierced must be None or lie in [0, 2^31), got 2147483648'),
    ('C.prune(pierced_ratio=0.5)', ValueError, 'pierced_ratio needs min_pierced >= 1'),
    ('C.prune(min_pierced=1, pierced_ratio=-1, before_stamp=1 << 31)', ValueError, 'pierced_ratio must be >= 0, got -1'),
    ('C.prune(min_pierced=1, pierced_ratio=nan)', ValueError, 'pierced_ratio must be >= 0, got nan'),
    ('C.prune(before_stamp=1 << 31, max_moving_fraction=nan)', ValueError, 'before_stamp must fit 32 bits, got 2147483648'),
    ('C.prune(before_stamp=-(1 << 31) - 1)', ValueError, 'before_stamp must fit 32 bits, got -2147483649'),
    ('C.prune(max_moving_fraction=nan, min_neighbors=-1)', ValueError, MMF),
    ('C.prune(min_neighbors=-1)', ValueError, 'min_neighbors must be None or lie in [0, 343], got -1'),
    ('C.prune(min_neighbors=344, radius=4)', ValueError, 'min_neighbors must be None or lie in [0, 343], got 344'),
    ('C.prune(min_neighbors=1, radius=4, box=3)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.prune(box=3)', ValueError, BOX + '3'),
    ('C.prune(box=((0, 0), (1, 1, 1)))', ValueError, BOX + '((0, 0), (1, 1, 1))'),
    ('C.prune(box=(("a", 0, 0), (1, 1, 1)))', ValueError, BOX + "(('a', 0, 0), (1, 1, 1))"),
    ('C.prune(box=((0, 0, nan), (1, 1, 1)))', ValueError, 'box: every bound must be finite, got ((0, 0, nan), (1, 1, 1))'),
    ('C.prune(box=((2, 0, 0), (1, 1, inf)))', ValueError, 'box: every bound must be finite, got ((2, 0, 0), (1, 1, inf))'),
    ('C.prune(box=((2, 0, 0), (1, 1, 1)))', ValueError, 'box: lo must not lie above hi, got ((2, 0, 0), (1, 1, 1))'),
    ('Ccpu.prune(radius=4, min_count=0)', native.NativeError, CLOUD_CPU),       # neither is checked: no min_neighbors, and prune has no check of min_count
    ('S.forget(before_stamp=1 << 31, box=3)', ValueError, 'before_stamp must fit 32 bits, got 2147483648'),
    ('S.forget(box=3)', ValueError, BOX + '3'),
    ('S.forget(box=((2, 0, 0), (1, 1, 1)))', ValueError, 'box: lo must not lie above hi, got ((2, 0, 0), (1, 1, 1))'),
    ('Scpu.forget()', native.NativeError, SPACE_CPU),
    # ---- components, planes
    ('C.components(radius=0)', ValueError, 'radius must be 1, 2 or 3 voxels, got 0'),
    ('C.components(radius=4, max_moving_fraction=nan)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.components(max_moving_fraction=nan, mask=F)', ValueError, MMF),
    ('C.components(mask=F)', ValueError, MASK),
    ('C.components(mask=B.reshape(1, 3))', ValueError, MASK),
    ('C.components(mask=B)', native.NativeError, 'components: mask must live on the GPU' + NO_CPU),
    ('Ccpu.components(min_count=0)', native.NativeError, CLOUD_CPU),
    ('C.remove_components()', ValueError, 'remove_components needs min_voxels or min_points'),
    ('C.remove_components(min_voxels=-1, radius=4)', ValueError, 'min_voxels and min_points must not be negative, got -1 0'),
    ('C.remove_components(min_points=-2)', ValueError, 'min_voxels and min_points must not be negative, got 0 -2'),
    ('C.remove_components(min_voxels=1, radius=4)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.remove_components(min_voxels=1, max_moving_fraction=nan)', ValueError, MMF),
    ('C.remove_components(min_voxels=1, mask=F)', ValueError, MASK),
    ('C.remove_components(min_voxels=1, mask=B)', native.NativeError, 'remove_components: mask must live on the GPU' + NO_CPU),
    ('Ccpu.remove_components(min_voxels=1)', native.NativeError, CLOUD_CPU),
    ('C.planes(radius=4, angle=91)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.planes(mask=B, angle=91)', native.NativeError, 'planes: mask must live on the GPU' + NO_CPU),
    ('C.planes(angle=91, max_offset=-1)', ValueError, 'angle must lie in [0, 90] degrees, got 91.0'),
    ('C.planes(angle=-1)', ValueError, 'angle must lie in [0, 90] degrees, got -1.0'),
    ('C.planes(max_offset=-1, max_variation=2)', ValueError, 'max_offset must be a distance in metres, not negative, got -1.0'),
    ('C.planes(max_variation=2, normals=3)', ValueError, 'max_variation must lie in [0, 1], got 2.0'),
    ('C.planes(normals=3)', ValueError, 'normals must be a result of normals(): a dict with normals, eigenvalues and flags'),
    ('C.planes(normals={"normals": P})', ValueError, 'normals must be a result of normals(): a dict with normals, eigenvalues and flags'),
    ('Ccpu.planes(min_count=0)', native.NativeError, CLOUD_CPU),
    ('C.plane_mask(1, angle=91)', ValueError, 'angle must lie in [0, 90] degrees, got 91.0'),
    ('C.split_planes(1, angle=91)', ValueError, 'angle must lie in [0, 90] degrees, got 91.0'),
    # ---- regrid, merge
    ('C.regrid()', ValueError, 'regrid needs a pose, a voxel_size or both'),
    ('C.regrid(capacity=0)', ValueError, 'regrid needs a pose, a voxel_size or both'),
    ('C.regrid(voxel_size=0, capacity=0)', ValueError, 'capacity must be at least the 0 rows of the map (the result never has more), got 0'),
    ('C.regrid(voxel_size=0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('C.regrid(voxel_size=0.2, capacity=(1 << 30) + 1)', ValueError, 'capacity must lie in [1, 2^30], got 1073741825'),
    ('C.regrid(pose=np.eye(3), voxel_size=0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('C.regrid(pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('Ccpu.regrid(pose=np.eye(4))', native.NativeError, CLOUD_CPU),
    ('S.regrid()', ValueError, 'regrid needs a pose, a voxel_size or both'),
    ('S.regrid(voxel_size=0, capacity=0)', ValueError, 'capacity must be at least the 0 rows of the table (the result never has more), got 0'),
    ('S.regrid(voxel_size=0)', ValueError, 'voxel_size must be a positive finite number, got 0.0'),
    ('S.regrid(voxel_size=0.2, capacity=(1 << 30) + 1)', ValueError, 'capacity must lie in [1, 2^30], got 1073741825'),
    ('S.regrid(pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('Scpu.regrid(pose=np.eye(4))', native.NativeError, SPACE_CPU),
    ('C.merge(3)', TypeError, 'merge takes an AccumulatedCloud, got int'),
    ('C.merge(S)', TypeError, 'merge takes an AccumulatedCloud, got ObservedSpace'),
    ('C.merge(Ccpu)', ValueError, 'merge: the maps live on cuda and cpu' + CARRIES),
    ('Ccpu.merge(C2)', ValueError, 'merge: the maps live on cpu and cuda' + CARRIES),
    ('C.merge(C2)', ValueError, 'merge: ' + VOXEL_SIZES + '; give pose= (np.eye(4) keeps the frame) or regrid() the other map first'),
    ('Ccpu.merge(Ccpu, pose=np.eye(3))', native.NativeError, CLOUD_CPU),        # a cloud looks at the pose only when it regrids
    ('S.merge(3)', TypeError, 'merge takes an ObservedSpace, got int'),
    ('S.merge(C)', TypeError, 'merge takes an ObservedSpace, got AccumulatedCloud'),
    ('S.merge(Scpu)', ValueError, 'merge: the maps live on cuda and cpu' + CARRIES),
    ('S.merge(S2)', ValueError, 'merge: ' + VOXEL_SIZES + '; give pose= (np.eye(4) keeps the frame) or regrid() the other map first'),
    ('S.merge(S2, pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('Scpu.merge(Scpu)', native.NativeError, SPACE_CPU),
    # ---- compare, select, difference
    ('C.compare(3)', TypeError, 'compare takes an AccumulatedCloud, got int'),
    ('C.compare(Ccpu)', ValueError, 'compare: the maps live on cuda and cpu' + CARRIES),
    ('C.compare(C2, max_distance=0)', ValueError, 'compare: ' + VOXEL_SIZES + "; regrid() one map onto the other's grid first"),
    ('C.compare(C, max_distance=0, min_count=0)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.0'),
    ('C.compare(C, max_distance=0.2)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.2'),
    ('C.compare(C, min_count=0)', ValueError, 'min_count must be at least 1, got 0'),
    ('C.compare(C, max_moving_fraction=nan)', ValueError, MMF),
    ('Ccpu.compare(Ccpu)', native.NativeError, CLOUD_CPU),
    ('C.difference(3)', TypeError, 'compare takes an AccumulatedCloud, got int'),
    ('C.difference(C, max_distance=0)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.0'),
    ('C.select(None)', ValueError, 'select needs a mask over the rows of extract()'),
    ('C.select(F, min_count=0)', ValueError, MASK),
    ('C.select(B, min_count=0)', native.NativeError, 'select: mask must live on the GPU' + NO_CPU),
    # ---- the observed space
    ('S.extract(min_rays=0)', ValueError, 'min_rays must be at least 1, got 0'),
    ('Scpu.extract(min_rays=0)', ValueError, 'min_rays must be at least 1, got 0'),
    ('S.occupancy(3, I)', TypeError, 'occupancy takes an AccumulatedCloud, got int'),
    ('S.occupancy(S, I)', TypeError, 'occupancy takes an AccumulatedCloud, got ObservedSpace'),
    ('S.occupancy(C2, I)', ValueError, 'occupancy: ' + VOXEL_SIZES),
    ('S.occupancy(Ccpu, I)', ValueError, 'occupancy: the cloud lives on cpu and the table on cuda'),
    ('S.occupancy(C, I)', native.NativeError, 'lookup_voxels: coords' + ON_GPU),
    # ---- load: CLOUD / SPACE write an .npz of two rows, with the arrays given in place of the good ones
    ('AccumulatedCloud.load(CLOUD(acc=np.zeros((5, 2), np.int32)))', ValueError, 'm.npz does not hold the records of an AccumulatedCloud'),
    ('AccumulatedCloud.load(CLOUD(stamps=np.zeros((2, 3), np.int32), keys=np.array([9, 5])))', ValueError,
     'm.npz does not hold the records of an AccumulatedCloud'),
    ('AccumulatedCloud.load(CLOUD(keys=np.array([9, 5]), pierced=np.zeros(2, np.int32)))', ValueError, 'm.npz: the keys are not ascending'),
    ('AccumulatedCloud.load(CLOUD(keys=np.array([5, 5])))', ValueError, 'm.npz: the keys are not ascending'),
    ('AccumulatedCloud.load(CLOUD(keys=np.array([-1, 5])))', ValueError, 'm.npz: the keys are not ascending'),
    ('AccumulatedCloud.load(CLOUD(pierced=np.zeros(2, np.int32)))', ValueError, 'm.npz does not hold the ray counts of an AccumulatedCloud'),
    ('AccumulatedCloud.load(CLOUD(pierced=np.zeros(3, np.int32), pierce_counters=np.zeros(5, np.int64)))', ValueError,
     'm.npz does not hold the ray counts of an AccumulatedCloud'),
    ('AccumulatedCloud.load(CLOUD(), "cpu")', native.NativeError, CLOUD_CPU),
    ('ObservedSpace.load(SPACE(rays=np.zeros(2, np.int32)))', ValueError, 'm.npz does not hold the columns of an ObservedSpace'),
    ('ObservedSpace.load(SPACE(counters=np.zeros(4, np.int64), keys=np.array([9, 5])))', ValueError, 'm.npz does not hold the columns of an ObservedSpace'),
    ('ObservedSpace.load(SPACE(keys=np.array([9, 5])))', ValueError, 'm.npz: the keys are not ascending'),
    ('ObservedSpace.load(SPACE(keys=np.array([-1, 5])))', ValueError, 'm.npz: the keys are not ascending'),
    ('ObservedSpace.load(SPACE(), "cpu")', native.NativeError, SPACE_CPU),
]

# The checks behind the scan: they need a tensor on the GPU to be reached.  No entry launches a kernel.
GPU_CASES = [
    ('C.add(P[:, :2])', ValueError, 'points must be [n,3], got (4, 2)'),
    ('C.add(P, moving=torch.zeros(4))', native.NativeError, 'add: moving must live on the GPU'),
    ('C.add(P, moving=B)', ValueError, 'moving must be [n], got (3,)'),
    ('C.register(P, max_distance=0, max_iter=-1)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.0'),
    ('C.register(P, max_distance=0.2)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.2'),
    ('C.register(P, max_iter=-1, radius=4)', ValueError, 'max_iter must lie in [0, 10000], got -1'),
    ('C.register(P, init_pose=np.eye(3), radius=4)', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('C.register(P, radius=4)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.query(P, max_distance=0.2, radius=4)', ValueError, 'max_distance must lie in (0, voxel_size = 0.1], got 0.2'),
    ('C.query(P, radius=4, min_neighbors=2)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
    ('C.query(P, min_neighbors=2, require_normal=True)', ValueError, 'min_neighbors must be at least 3, got 2'),
    ('C.query(P, require_normal=True, pose=np.eye(3))', ValueError, 'require_normal=True needs normals=True'),
    ('C.query(P, pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('C.knn(P, 0, pose=np.eye(3))', ValueError, 'k must lie in [1, 16], got 0'),
    ('C.knn(P, 1, radius=5)', ValueError, 'radius must lie in [1, 4] voxels, got 5'),
    ('C.see_through(P, np.zeros((2, 2)), margin=-1)', ValueError, 'origins must be [3] or [S,3] with S >= 1, got (2, 2)'),
    ('C.see_through(P, np.zeros(3), origin_index=torch.zeros(4))', native.NativeError, 'see_through: origin_index must live on the GPU'),
    ('C.see_through(P, np.zeros(3), margin=-1, max_range=-1)', ValueError, 'margin must be a finite number >= 0, got -1.0'),
    ('C.see_through(P, np.zeros(3), margin=inf)', ValueError, 'margin must be a finite number >= 0, got inf'),
    ('C.see_through(P, np.zeros(3), max_range=-1, max_steps=0)', ValueError, 'max_range must be >= 0 or None, got -1'),
    ('C.see_through(P, np.zeros(3), max_range=nan)', ValueError, 'max_range must be >= 0 or None, got nan'),
    ('C.see_through(P, np.zeros(3), max_steps=0, pose=np.eye(3))', ValueError, 'max_steps must lie in [1, 2^16], got 0'),
    ('C.see_through(P, np.zeros(3), max_steps=(1 << 16) + 1)', ValueError, 'max_steps must lie in [1, 2^16], got 65537'),
    ('C.see_through(P, np.zeros(3), pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('C.raycast(P, np.zeros((2, 2)), min_range=-1)', ValueError, 'origins must be [3] or [S,3] with S >= 1, got (2, 2)'),
    ('C.raycast(P, np.zeros(3), min_range=-1, margin=-1)', ValueError, 'min_range must be a finite number >= 0, got -1.0'),
    ('C.raycast(P, np.zeros(3), margin=-1, max_range=-1)', ValueError, 'margin must be a finite number >= 0, got -1.0'),
    ('C.raycast(P, np.zeros(3), max_range=-1, margin=0.1)', ValueError, 'max_range must be >= 0 or None, got -1.0'),
    ('C.raycast(P, np.zeros(3), max_range=5, margin=0.1, max_steps=0)', ValueError,
     'margin is measured from the target: it cannot be combined with a max_range'),
    ('C.raycast(P, np.zeros(3), max_steps=0, pose=np.eye(3))', ValueError, 'max_steps must lie in [1, 2^16], got 0'),
    ('C.raycast(P, np.zeros(3), pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('S.observe(P, np.zeros((2, 2)), margin=-1)', ValueError, 'origins must be [3] or [S,3] with S >= 1, got (2, 2)'),
    ('S.observe(P, np.zeros(3), margin=-1, max_range=-1)', ValueError, 'margin must be a finite number >= 0, got -1.0'),
    ('S.observe(P, np.zeros(3), max_range=-1, max_steps=0)', ValueError, 'max_range must be >= 0 or None, got -1'),
    ('S.observe(P, np.zeros(3), max_steps=0, stamp=1 << 31)', ValueError, 'max_steps must lie in [1, 2^16], got 0'),
    ('ObservedSpace(0.1, DEV, 64, visit_budget=8).observe(P, np.zeros(3), max_steps=16, stamp=1 << 31)', ValueError,
     'visit_budget 8 is below max_steps 16: a single ray must fit'),
    ('S.observe(P, np.zeros(3), stamp=1 << 31, pose=np.eye(3))', ValueError, 'stamp must fit 32 bits, got 2147483648'),
    ('S.observe(P, np.zeros(3), pose=np.eye(3))', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('S.lookup(P, min_rays=0, pose=np.eye(3))', ValueError, 'min_rays must be at least 1, got 0'),
    ('S.lookup_voxels(F.reshape(1, 3), min_rays=0)', ValueError, 'coords must be int32 or int64 voxel indices, got torch.float32'),
    ('S.lookup_voxels(I, min_rays=0)', ValueError, 'min_rays must be at least 1, got 0'),
    ('C.clearance(coords=F.reshape(1, 3))', ValueError, 'coords must be int32 or int64 voxel indices, got torch.float32'),
    ('C.clearance(points=P, pose=np.eye(3), field=FIELD, planar=True)', ValueError, 'pose must be [4,4], got (3, 3)'),
    ('C.clearance(points=P, field=FIELD, planar=True)', ValueError, "clearance: a field and arguments for a new one: ['planar']"),
    ('C.select(B, min_count=0, capacity=0)', ValueError, 'min_count must be at least 1, got 0'),
    ('C.select(B, max_moving_fraction=nan)', ValueError, MMF),
    ('C.select(B, capacity=0)', ValueError, 'capacity must be at least the 0 rows of the map (the result never has more), got 0'),
    ('C.select(B, capacity=(1 << 30) + 1)', ValueError, 'capacity must lie in [1, 2^30], got 1073741825'),
    ('C.components(mask=B, radius=4)', ValueError, 'radius must be 1, 2 or 3 voxels, got 4'),
]


def _npz(good):
    def write(**arrays):
        with open('m.npz', 'wb') as f:
            np.savez(f, **dict(good, **arrays))
        return 'm.npz'
    return write


def _namespace(device):
    """What the expressions of the tables see; `device` is where the maps and the tensors live."""
    tensor_device = 'cpu' if device == 'cuda' else device                      # the CPU table: maps that say 'cuda' and tensors that are not there
    rows = dict(keys=np.array([5, 9], np.int64), stamps=np.zeros((2, 2), np.int32), voxel_size=np.float64(0.1))
    P = torch.zeros((4, 3), device=tensor_device)
    return dict(
        AccumulatedCloud=AccumulatedCloud, ObservedSpace=ObservedSpace, np=np, torch=torch, nan=float('nan'), inf=float('inf'), DEV=DEV,
        C=AccumulatedCloud(0.1, device, 64), C2=AccumulatedCloud(0.2, device, 64), Ccpu=AccumulatedCloud(0.1, 'cpu', 64),
        S=ObservedSpace(0.1, device, 64), S2=ObservedSpace(0.2, device, 64), Scpu=ObservedSpace(0.1, 'cpu', 64),
        P=P, I=torch.zeros((4, 3), dtype=torch.int32, device=tensor_device), B=torch.zeros((3,), dtype=torch.bool, device=tensor_device),
        F=torch.zeros((3,), device=tensor_device), R2={'rec_est': P, 'mos_est': torch.zeros((4, 2), device=tensor_device), '_n_batches': 2},
        D={'time_indice': torch.zeros((4, 2), device=tensor_device)}, FIELD={'max_radius': 1, 'dist2': torch.zeros((1, 1, 1), dtype=torch.int32)},
        CLOUD=_npz(dict(rows, acc=np.zeros((5, 2), np.int64), dropped=np.int64(0))),
        SPACE=_npz(dict(rows, rays=np.ones((2,), np.int64), counters=np.zeros((5,), np.int64))))


def _raises(expression, exception, message, device, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                                 # CLOUD and SPACE write m.npz
    with pytest.raises(exception) as e:
        eval(expression, _namespace(device))
    assert type(e.value) is exception and str(e.value) == message


@pytest.mark.parametrize('expression,exception,message', CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_argument_checks(expression, exception, message, tmp_path, monkeypatch):
    """Every check that fires before device memory is taken: type and text as they were before the classes had a base, and -- where an expression
    breaks two rules -- the one that fired first."""
    _raises(expression, exception, message, 'cuda', tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('expression,exception,message', GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_argument_checks_gpu(expression, exception, message, tmp_path, monkeypatch):
    _raises(expression, exception, message, DEV, tmp_path, monkeypatch)


# ---- structure -----------------------------------------------------------------------------------------------------------------------------
ONCE = ('while True:', '_alt = None', '<< 42', '>> 42', 'max_distance must lie in (0, voxel_size', 'margin must be a finite', 'max_range must be >= 0',
        'max_steps must lie in', 'radius must be 1, 2 or 3', 'min_neighbors must be at least 3', 'max_moving_fraction must be a number', 'must fit 32 bits',
        'capacity must be at least the', 'save() / load() carries', 'the keys are not ascending')


def test_one_copy_of_the_table_scaffolding():
    """What AccumulatedCloud and ObservedSpace share stands once, in _VoxelTable or in a module function: the double-table growth loop and the staging
    of _alt, the packing of a voxel key and its inverse, and every argument check that several methods make.  voxel_mean_downsample keeps its own
    `capacity *= 2`."""
    text = open(os.path.join(ROOT, 'pcaccumulation_amd', 'accumulate.py')).read()
    for phrase in ONCE:
        assert text.count(phrase) == 1, phrase
    assert issubclass(AccumulatedCloud, accumulate._VoxelTable) and issubclass(ObservedSpace, accumulate._VoxelTable)
    space = text[text.index('\nclass ObservedSpace('):]
    space = space[:re.search(r'\n\n\n(?=\S)', space).start()]                   # up to the next definition at module level: the end of the class
    assert 'isinstance(cloud, AccumulatedCloud)' in space
    assert 'AccumulatedCloud.' not in re.sub(r'""".*?"""', '', space, flags=re.S)    # outside the docstrings: no borrowed method


# ---- the call transcript -------------------------------------------------------------------------------------------------------------------
_OUTPUTS = ('counters', 'out', 'out_a', 'out_b', 'n')                           # torch.empty results: the values before the call mean nothing


def _describe(v, values=True):
    """An argument as JSON: None; a tensor as dtype and shape, with the values when it has at most 16 elements (floats as hex: exact, nan included);
    tuples and lists element-wise; the tensors of a dict by dtype and shape; any scalar by repr."""
    if v is None:
        return None
    if torch.is_tensor(v):
        d = {'dtype': str(v.dtype), 'shape': list(v.shape)}
        if values and v.numel() <= 16:
            d['values'] = [x.hex() if isinstance(x, float) else int(x) for x in v.detach().cpu().reshape(-1).tolist()]
        return d
    if isinstance(v, (tuple, list)):
        return [_describe(x, values) for x in v]
    if isinstance(v, dict):
        return {k: _describe(x, False) for k, x in sorted(v.items())}
    return repr(v)


def _record_calls(setattr_, transcript):
    """Replaces every native.accum_* by a function that notes the call -- the name and every argument under its parameter's name -- and calls
    through."""
    def recorder(name, fn):
        signature = inspect.signature(fn)

        def call(*args, **kw):
            bound = signature.bind(*args, **kw).arguments
            transcript.append([name, {k: _describe(v, k not in _OUTPUTS) for k, v in bound.items()}])
            return fn(*args, **kw)
        return call
    for name in sorted(vars(native)):
        if name.startswith('accum_') and inspect.isfunction(getattr(native, name)):
            setattr_(native, name, recorder(name, getattr(native, name)))


def _digest(arrays):
    """records() as shapes and a hash of the bytes: equal exactly when every integer is."""
    return [[str(a.dtype), list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()] for a in arrays]


def _session(folder):
    """Two clouds and two spaces through every method, from three windows of accumulate_helpers.window() at voxel size 0.5 (12 x 12 x 6 voxels hold the
    points: nearly every voxel has neighbours) and capacity 64 (every first call has to grow).  -> (the integer dicts the methods returned, the
    records of every map and table at the end, each by name)."""
    VS = 0.5
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    scans = [(up(pts[:2000]), up(mv[:2000]), stamp, pose) for pts, mv, stamp, pose in (ah.window(k) for k in range(3))]
    (p0, m0, t0, T0), (p1, m1, t1, T1), (p2, m2, t2, T2) = scans
    sensor = np.array([[0.05, -0.02, 0.3], [0.3, 0.1, 0.25]])
    index = (torch.arange(p1.shape[0], device=DEV) % 2).to(torch.int64)
    got, maps = {}, {}

    m = AccumulatedCloud(VS, DEV, 64)
    m.add(p0, T0, m0, t0)                                                       # grows by doubling
    m.see_through(p1, sensor, index, T1, m1, stamp=t1, max_steps=256)
    m.add(p1, T1, m1, t1)                                                       # carries the ray counts
    m.extract(min_count=2, max_moving_fraction=0.5)
    m.pierced(min_count=2)
    m.query(p2, T2, max_distance=0.4, min_count=2, normals=True, require_normal=True, viewpoints=sensor)
    m.query(p2)
    m.knn(p2, 4, T2, radius=2, min_count=2)
    m.neighbors(4, radius=1)
    m.raycast(p2, sensor, index, T2, max_range=6.0, min_range=0.5, min_count=2, max_steps=128)
    m.raycast(p2, sensor[0], margin=0.25)
    m.normals(radius=2, min_neighbors=4, min_count=2, viewpoints=sensor, stamp_base=1)
    m.register(p2, T2, m2, max_iter=2, min_count=2, radius=1, min_neighbors=4)
    got['prune_dry'] = m.prune(min_pierced=2, pierced_ratio=0.25, before_stamp=1, min_count=2, max_moving_fraction=0.9, min_neighbors=3, radius=1,
                               box=((-2.9, -2.9, -1.4), (2.9, 2.9, 1.4)), dry_run=True)
    got['prune'] = m.prune(min_pierced=2, pierced_ratio=0.25, min_count=2, min_neighbors=3, radius=1, box=((-2.9, -2.9, -1.4), (2.9, 2.9, 1.4)))
    mask = m.extract()['coords'][:, 2] > -2
    m.components(radius=1, mask=mask)
    got['remove_dry'] = m.remove_components(min_voxels=4, min_points=8, min_count=2, mask=mask[:m.extract(min_count=2)['coords'].shape[0]], dry_run=True)
    got['remove'] = m.remove_components(min_voxels=4, min_points=8, min_count=2, mask=mask[:m.extract(min_count=2)['coords'].shape[0]])
    got['remove_none'] = m.remove_components(min_voxels=4, radius=1)
    m.planes(angle=20.0, max_variation=0.2, radius=1, normal_radius=1, min_neighbors=4)
    m.columns(ground_radius=1, thickness=1, band=(1, 4), min_count=2)
    m.bev(band=(1, 4))
    m.bev(origin=(-4, -5), shape=(9, 8), min_count=2)
    field = m.distance_field(max_radius=4)
    m.distance_field(origin=(-5, -5, -2), shape=(10, 10, 3), max_radius=3, planar=True, min_count=2)
    m.distance_field(origin=(-5, -5, -2), max_radius=2, pad=False)
    m.clearance(points=p2, pose=T2, field=field)
    m.clearance(coords=m.extract()['coords'][:50].to(torch.int64), max_radius=2)
    other = AccumulatedCloud(VS, DEV, 64).add(p2, T2, m2, t2)
    got['compare'] = m.compare(other, max_distance=0.3, min_count=2)['counters']
    top = m.select(m.extract(min_count=2)['coords'][:, 2] >= 0, min_count=2, capacity=1024)
    bottom = m.select(m.extract()['coords'][:, 2] >= 0, invert=True)
    gone = m.difference(other, max_distance=0.3)
    turned = m.regrid(pose=ah.rot_axis((0, 0, 1), 0.3, (0.2, 0.0, 0.1)), capacity=4096)
    coarse = m.regrid(voxel_size=1.0)
    clone = m.copy()
    got['merge'] = m.merge(other)
    got['merge_empty'] = m.merge(AccumulatedCloud(VS, DEV, 64))
    small = AccumulatedCloud(VS, DEV, 64).add(p0[:40], T0)
    got['merge_grows'] = small.merge(m)                                         # grows, and takes ray counts it did not have
    got['merge_posed'] = clone.merge(coarse, pose=ah.rot_axis((0, 1, 0), 0.1, (0.0, 0.3, 0.0)))
    m.save(os.path.join(folder, 'm.npz'))
    loaded = AccumulatedCloud.load(os.path.join(folder, 'm.npz'), DEV)
    loaded.add(p0, T0, m0, 12)                                                  # a loaded map goes on: state words and ray counts are in place
    AccumulatedCloud(VS, DEV, 64).add(p0[:100]).save(os.path.join(folder, 'plain.npz'))     # without ray counts
    plain = AccumulatedCloud.load(os.path.join(folder, 'plain.npz'), DEV)
    maps.update(m=m, other=other, top=top, bottom=bottom, gone=gone, turned=turned, coarse=coarse, clone=clone, small=small, loaded=loaded, plain=plain)

    s = ObservedSpace(VS, DEV, 64, visit_budget=4096)
    s.observe(p0, sensor, None, T0, m0, t0, max_steps=64)                       # grows, and the rays are cut for the visit budget
    s.observe(p1, sensor, index, T1, m1, t1, margin=0.25, max_range=4.0, max_steps=64)
    got['splits'] = s.splits
    got['counters'] = s.counters
    s.extract(min_rays=2)
    s.lookup(p2, T2, min_rays=2)
    coords = m.extract()['coords']
    s.lookup_voxels(coords)
    s.lookup_voxels(coords.to(torch.int64), min_rays=3)
    s.occupancy(m, coords, min_count=2, min_rays=2)
    s2 = ObservedSpace(VS, DEV, 64, visit_budget=1 << 20).observe(p2, sensor[1], None, T2, m2, t2, max_steps=64)
    both = s.copy()
    got['space_merge'] = both.merge(s2)
    got['space_merge_empty'] = both.merge(ObservedSpace(VS, DEV, 64))
    few = ObservedSpace(VS, DEV, 64).observe(p1[:8], sensor[1], None, T1, None, t1, max_steps=64)
    got['space_merge_grows'] = few.merge(both)                                  # grows
    far = s2.regrid(pose=ah.rot_axis((0, 0, 1), 0.3, (0.5, 0.0, 0.0)), voxel_size=1.0)
    got['space_merge_posed'] = s.merge(s2, pose=ah.rot_axis((0, 0, 1), 0.05, (0.0, 0.1, 0.0)))
    got['forget'] = s.forget(before_stamp=1, box=((-2.0, -2.0, -1.0), (2.0, 2.0, 1.0)))
    got['forget_none'] = s.forget()
    s.save(os.path.join(folder, 's.npz'))
    again = ObservedSpace.load(os.path.join(folder, 's.npz'), DEV)
    again.observe(p0[:300], sensor[0], stamp=9, max_steps=64)
    got['dropped_rows'] = far.dropped_rows
    maps.update(s=s, s2=s2, both=both, few=few, far=far, again=again)
    state = {name: [t.num_voxels, t.capacity, getattr(t, 'dropped', None), None if getattr(t, '_pierced', None) is None else
                    int(t._pierced[:t.num_voxels].sum()), getattr(t, '_counters', None) if isinstance(t, ObservedSpace) else None]
             for name, t in maps.items()}
    return got, {name: _digest(t.records()) for name, t in maps.items()}, state


N_CALLS = 87                                                                   # the length of the session's transcript


def _run(setattr_, folder):
    transcript = []
    _record_calls(setattr_, transcript)
    got, records, state = _session(str(folder))
    return json.loads(json.dumps(dict(calls=len(transcript), returned=got, state=state, records=records, transcript=transcript)))


def _module_sha256():
    with open(accumulate.__file__.replace('.pyc', '.py'), 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()


def _dump(result, f):
    """The golden file: one line per part, one line per call of the transcript."""
    parts = ['"%s": %s' % (k, json.dumps(result[k], sort_keys=True)) for k in sorted(result) if k != 'transcript']
    calls = ',\n  '.join(json.dumps(c, sort_keys=True) for c in result['transcript'])
    f.write('{\n' + ',\n'.join(parts) + ',\n"transcript": [\n  ' + calls + '\n]\n}\n')


@pytest.mark.gpu
def test_call_transcript_gpu(tmp_path, monkeypatch):
    """The session makes the native calls it made at the recorded commit, in that order and with those arguments, returns the same integers and leaves
    the same records in every map and table."""
    now = _run(monkeypatch.setattr, tmp_path)
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden['recorded_at'] == RECORDED_AT and golden['recorded_from'] == RECORDED_FROM
    for at, (a, b) in enumerate(zip(now['transcript'], golden['transcript'])):
        assert a == b, 'call %d: %s' % (at, a[0])
    assert now['calls'] == golden['calls'] == N_CALLS
    for part in ('returned', 'state', 'records'):
        assert now[part] == golden[part], part
    again = [c[0] for a, c in zip(now['transcript'], now['transcript'][1:]) if a[0] == c[0] and a[1].get('tables_out') != c[1].get('tables_out')]
    assert {'accum_add', 'accum_merge', 'accum_observe', 'accum_observed_merge'} <= set(again)      # each made an attempt again with larger tables
    assert now['returned']['splits'] >= 1                                       # and a call's rays were cut for the visit budget


if __name__ == '__main__':
    import tempfile
    assert sys.argv[1:] == ['--record'], 'usage: python tests/test_accumulate_host.py --record   (on a GPU, at the commit RECORDED_AT names)'
    # the golden file is what THAT commit's accumulate.py does: a recording from any other text of the module would only agree with itself
    assert _module_sha256() == RECORDED_FROM, 'pcaccumulation_amd/accumulate.py is not the file of commit %s (sha256 %s)' % (RECORDED_AT, RECORDED_FROM)
    with tempfile.TemporaryDirectory() as tmp:
        result = _run(setattr, tmp)
    with open(GOLDEN, 'w') as f:
        _dump(dict(result, recorded_at=RECORDED_AT, recorded_from=RECORDED_FROM), f)
    print('%s: %d calls' % (GOLDEN, result['calls']))
