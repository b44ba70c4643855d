"""Test-time ICP pose refinement (model.ego_icp, model.tpointnet_icp): the segment and job tables of the two call sites for
native.icp_point_to_point (include/pcacc.h C3).  The reference runs Open3D's registration_icp on the host, once per frame
(models/egomotion.py:360-384) and once per frame of every instance (models/alignnet.py:54-112); here each call site is ONE batched call and nothing
comes back to the host."""
import torch

from . import native

MAX_SEGMENTS = 65535               # include/pcacc.h C3: the segment shares the 64-bit cell key


class IcpError(RuntimeError):
    pass


def segments_by_key(points, key, n_keys):
    """points [N,3], key [N] in [0, n_keys) or negative (the point takes part in nothing) -> (points grouped by key [N,3] f32, offsets [n_keys+1] i32):
    a stable sort, so that the order inside a segment is the input's (a tie between equal distances goes to the lowest index).  No host sync."""
    if n_keys > MAX_SEGMENTS:
        raise IcpError('ICP: %d segments, the kernel takes %d per call' % (n_keys, MAX_SEGMENTS))
    key = key.long()
    key = torch.where(key >= 0, key, torch.full_like(key, n_keys))
    order = torch.argsort(key, stable=True)
    grouped = points.detach().float().index_select(0, order).contiguous()
    counts = torch.zeros(n_keys + 1, dtype=torch.int64, device=points.device).index_add_(0, key, torch.ones_like(key))
    offsets = torch.cat((torch.zeros(1, dtype=torch.int64, device=points.device), torch.cumsum(counts[:n_keys], 0)))
    return grouped, offsets.to(torch.int32)


def anchor_jobs(n_groups, T, device):
    """{source = frame t, target = frame 0} of every group (sample or instance), t = 1 .. T-1; segment = group * T + frame."""
    jobs = [(g * T + t, g * T) for g in range(n_groups) for t in range(1, T)]
    return native.upload_small(jobs, torch.int32, device).view(-1, 2)


def refine_ego_poses(points, frame_idx, background, chained, B, T, threshold, max_iter):
    """models/egomotion.py:360-384 for all samples: points [N,3] raw input points, frame_idx [N] = sample * T + frame, background [N] bool
    (fb_est_per_point == 0), chained [B*T,4,4] the sequence estimate -> (refined [B*T,4,4] f32 with frame 0 = identity, status [B*(T-1)] i32)."""
    dev = points.device
    key = torch.where(background, frame_idx.long(), torch.full_like(frame_idx.long(), -1))
    grouped, offsets = segments_by_key(points, key, B * T)
    init = chained.detach().view(B, T, 4, 4)[:, 1:].reshape(-1, 4, 4).double().contiguous()
    pose, _, _, _, status = native.icp_point_to_point(grouped, offsets, anchor_jobs(B, T, dev), init, threshold, max_iter)
    refined = torch.eye(4, device=dev).repeat(B, T, 1, 1)
    refined[:, 1:] = pose.float().view(B, T - 1, 4, 4)                    # float64 product, cast once (egomotion.py:25-26)
    return refined.view(B * T, 4, 4), status


def refine_instance_poses(points, frames, labels, pose_est, threshold, max_iter=50):
    """models/alignnet.py:95-112: points [N,3] (padded: every instance has frame-0 points), frames [N], labels [N] in [0,K), pose_est [K,T,4,4]
    -> (refined @ pose_est [K,T,4,4], empty-anchor flag 0-d i32, status [K*(T-1)] i32).  The target of every frame is the instance's frame 0 alone (the reference never
    grows its accumulated cloud); frames without points keep the identity."""
    from .tpointnet import reconstruct_sequence
    K, T = pose_est.shape[0], pose_est.shape[1]
    dev = points.device
    rec = reconstruct_sequence(points, frames, labels, pose_est.detach(), T)
    grouped, offsets = segments_by_key(rec, labels.long() * T + frames.long(), K * T)
    pose, _, _, _, status = native.icp_point_to_point(grouped, offsets, anchor_jobs(K, T, dev), None, threshold, max_iter)
    refined = torch.eye(4, device=dev).repeat(K, T, 1, 1)
    refined[:, 1:] = pose.float().view(K, T - 1, 4, 4)
    # run_icp asserts a populated frame 0 (alignnet.py:63-64); padding() guarantees it, the kernel reports it: a job whose source has points but
    # whose anchor is empty
    anchor_empty = ((status & native.ICP_EMPTY_TARGET) != 0) & ((status & native.ICP_EMPTY_SOURCE) == 0)
    return torch.matmul(refined, pose_est.float()), anchor_empty.any().to(torch.int32), status


def guarded(copy, index, convert):
    """`convert` of a lazy.LazyValue, refusing when element `index` of the same transfer says an instance had no anchor-frame points."""
    def checked(values):
        if copy.numpy()[index] != 0:
            raise IcpError('model.tpointnet_icp: an instance has points but none in frame 0 (models/alignnet.py:63-64 asserts this)')
        return convert(values)
    return checked
