"""The pointops module on the gfx950 kernels: every name of cpp/pointops/functions/pointops.py with its signature.

The Functions are amcontrast3d_amd.ops.KNNQuery and the offset-layout operators of amcontrast3d_amd.offset_ops
(csrc/pointops.hip); `querygroup`, `queryandgroup` and `interpolation` are the reference's compositions around them
(pointops.py:112-178, 251-265), with the neighbour gathers going through `grouping` (the same values; the gradient is
the same sum).  Kept as the reference has them: `querygroup` returns nothing when an `idx` is passed in, normalises each
neighbour offset by its own norm (+1e-8) only when `query_method == 'knn'` exactly and by `radius` otherwise, and its
`nsample is None` branch is the torch expression that fails on 2-D input; `queryandgroup(use_xyz=False)` returns the
features alone.  Only ``knnquery`` is reached from the AMContrast3D path.
"""
import torch

from amcontrast3d_amd.offset_ops import (  # noqa: F401
    Aggregation, BallQuery, FurthestSampling, Grouping, Interpolation, Subtraction, aggregation, ballquery, furthestsampling,
    grouping, interpolation2, subtraction)
from amcontrast3d_amd.ops import KNNQuery, knnquery  # noqa: F401


def querygroup(nsample, xyz, new_xyz, feat, offset, new_offset,
               radius=None, query_method='knn',
               normalize_dp=False, idx=None
               ):
    """k-NN (`query_method` 'knn' / 'knnquery') or ball neighbourhoods of new_xyz (m,3) in xyz (n,3) per segment, gathered:
    -> (neighbour positions relative to their query (m,nsample,3), neighbour features (m,nsample,c) or None)"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    if new_xyz is None:
        new_xyz = xyz
    if idx is not None:
        return None  # the reference's function ends without a return on this path
    if nsample is None:  # "group all": the torch expression, which fails on (n, 3) input there and here
        dp = xyz.transpose(1, 2).unsqueeze(2)
        return dp, (feat.unsqueeze(2) if feat is not None else None)
    if query_method in ('knn', 'knnquery'):
        idx = knnquery(nsample, xyz, new_xyz, offset, new_offset)[0]
    else:
        idx = ballquery(radius, nsample, xyz, new_xyz, offset, new_offset)
    dp = grouping(xyz, idx)  # (m, nsample, 3)
    dp -= new_xyz.unsqueeze(1)
    if normalize_dp:
        if query_method == 'knn':  # exactly 'knn': the maximum runs over an axis of size 1, so every offset gets unit norm
            scale = dp.norm(dim=-1, p=2, keepdim=True).max(dim=-1, keepdim=True)[0] + 1.0e-8
        else:
            scale = radius
        dp /= scale
    return dp, (grouping(feat, idx) if feat is not None else None)


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """the neighbourhoods `idx` (m,nsample), or the k-NN ones when it is None, gathered: relative positions and features
    concatenated (m,nsample,3+c), or the features alone (m,nsample,c) without use_xyz"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    if new_xyz is None:
        new_xyz = xyz
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)  # (m, nsample)
    idx = idx.view(new_xyz.shape[0], nsample).to(torch.int32).contiguous()
    grouped_xyz = grouping(xyz, idx)  # (m, nsample, 3)
    grouped_xyz -= new_xyz.unsqueeze(1)
    grouped_feat = grouping(feat, idx)  # (m, nsample, c)
    if use_xyz:
        return torch.cat((grouped_xyz, grouped_feat), -1)  # (m, nsample, 3+c)
    else:
        return grouped_feat


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """feat (m,c) at xyz (m,3) carried to new_xyz (n,3) by inverse-distance weights over the k nearest rows of the same
    segment, as a loop over k in torch -> (n,c); `interpolation2` is the same on the kernels"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)  # (n, k) each
    w = 1.0 / (dist + 1e-8)
    w = w / torch.sum(w, dim=1, keepdim=True)
    out = torch.zeros(new_xyz.shape[0], feat.shape[1], dtype=torch.float32, device=feat.device)
    for t in range(k):
        out += feat[idx[:, t].long(), :] * w[:, t].unsqueeze(-1)
    return out
