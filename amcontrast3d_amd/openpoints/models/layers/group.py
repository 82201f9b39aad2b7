"""Neighbourhood grouping layers on the gfx950 kernels.

API mirror of models/layers/group.py: ``ball_query``, ``grouping_operation``,
``gather_operation``, ``QueryAndGroup`` (:206-255), ``GroupAll`` (:258-272),
``get_aggregation_feautres`` (:323-335, name kept as spelled there),
``create_grouper`` (:338-352), ``torch_grouping_operation`` (:120-137), ``KNN`` (:12-28), ``DenseDilated`` (:31-54),
``DilatedKNN`` (:57-73), ``KNNGroup`` (:275-320).
"""
import copy
import logging

import torch
import torch.nn as nn

from amcontrast3d_amd.ops import ball_query, gather_operation, grouping_operation, knn_group_dp
from .knn import DenseDilated, kernel_route, kernel_search


class KNN(nn.Module):
    """group.py's own KNN: forward(support, query) -> distances (B,k,M) -- topk(dim=1) values, left untransposed as the
    reference leaves them -- and indices (B,M,k) int32.  Routes as in layers/knn.py."""

    def __init__(self, neighbors, transpose_mode=True):
        super(KNN, self).__init__()
        self.neighbors = neighbors

    @torch.no_grad()
    def forward(self, support, query):
        if kernel_route(query, support, self.neighbors):
            return kernel_search(self.neighbors, query, support, dist="bkm")
        dist = torch.cdist(support, query)
        k_dist = dist.topk(k=self.neighbors, dim=1, largest=False)
        return k_dist.values, k_dist.indices.transpose(1, 2).contiguous().int()


class DilatedKNN(nn.Module):
    """indices (B,N,k) int32 of the dilated k-NN of a cloud among itself"""

    def __init__(self, k=9, dilation=1, stochastic=False, epsilon=0.0):
        super(DilatedKNN, self).__init__()
        self.dilation = dilation
        self.stochastic = stochastic
        self.epsilon = epsilon
        self.k = k
        self._dilated = DenseDilated(k, dilation, stochastic, epsilon)
        self.knn = KNN(k * self.dilation, transpose_mode=True)

    def forward(self, query):
        if not kernel_route(query, query, self.k * self.dilation):
            _, idx = self.knn(query, query)
            return self._dilated(idx)
        randnum = self._dilated.draw()  # the reference's draws, in its order; the strided pick is the search's epilogue
        if randnum is None:
            return kernel_search(self.k, query, query, dilation=self.dilation)[1]
        return self._dilated.pick(kernel_search(self.k * self.dilation, query, query)[1], randnum)


def torch_grouping_operation(features, idx):
    """pure-torch gather: (B,C,N), (B,npoint,nsample) -> (B,C,npoint,nsample)"""
    B, C = features.shape[:2]
    flat = idx.reshape(B, 1, -1).expand(-1, C, -1).long()
    return features.gather(2, flat).reshape(B, C, idx.shape[1], idx.shape[2])


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, relative_xyz=True, normalize_dp=False, normalize_by_std=False,
                 normalize_by_allstd=False, normalize_by_allstd2=False, return_only_idx=False, **kwargs):
        super().__init__()
        self.radius, self.nsample = radius, nsample
        self.normalize_dp = normalize_dp
        self.normalize_by_std = normalize_by_std
        self.normalize_by_allstd = normalize_by_allstd
        self.normalize_by_allstd2 = normalize_by_allstd2
        assert self.normalize_dp + self.normalize_by_std + self.normalize_by_allstd < 2
        self.relative_xyz = relative_xyz
        self.return_only_idx = return_only_idx

    def query(self, query_xyz, support_xyz):
        """neighbour indices (B,npoint,nsample) int32 -- geometry only"""
        return ball_query(self.radius, self.nsample, support_xyz, query_xyz)

    def relative_positions(self, idx, query_xyz, support_xyz):
        """(B,3,npoint,nsample) neighbour offsets, divided by the radius if normalize_dp -- geometry only"""
        grouped_xyz = grouping_operation(support_xyz.transpose(1, 2).contiguous(), idx)
        if self.relative_xyz:
            grouped_xyz = grouped_xyz - query_xyz.transpose(1, 2).unsqueeze(-1)
            if self.normalize_dp:
                grouped_xyz /= self.radius
        return grouped_xyz

    def forward(self, query_xyz, support_xyz, features=None, geom=None):
        """query (B,npoint,3), support (B,N,3), features (B,C,N)
        -> relative positions (B,3,npoint,nsample), grouped features (B,C,npoint,nsample).
        `geom` = {'idx', 'dp'} precomputed by query()/relative_positions() (they do not depend on the
        features, so a caller may prepare them ahead of time / on another stream)."""
        idx = geom['idx'] if geom is not None else self.query(query_xyz, support_xyz)
        if self.return_only_idx:
            return idx
        grouped_xyz = geom['dp'] if geom is not None else self.relative_positions(idx, query_xyz, support_xyz)
        grouped_features = grouping_operation(features, idx) if features is not None else None
        return grouped_xyz, grouped_features


class KNNGroup(nn.Module):
    """The k nearest support points of every query, QueryAndGroup's protocol: query() and relative_positions() are the
    coordinate-only halves a caller may run ahead of time (`geom`)."""

    def __init__(self, nsample, relative_xyz=True, normalize_dp=False, return_only_idx=False, **kwargs):
        super().__init__()
        self.nsample = nsample
        self.knn = KNN(nsample, transpose_mode=True)
        self.relative_xyz = relative_xyz
        self.normalize_dp = normalize_dp
        self.return_only_idx = return_only_idx

    def query(self, query_xyz, support_xyz):
        """neighbour indices (B,npoint,nsample) int32 -- geometry only"""
        if kernel_route(query_xyz, support_xyz, self.nsample):
            return kernel_search(self.nsample, query_xyz, support_xyz)[1]  # no distances wanted: none written
        return self.knn(support_xyz, query_xyz)[1]

    @torch.no_grad()
    def relative_positions(self, idx, query_xyz, support_xyz):
        """(B,3,npoint,nsample) neighbour offsets; normalize_dp divides every cloud by its largest offset length (taken
        after the subtraction, and without relative_xyz too, group.py:312-315) -- geometry only"""
        if kernel_route(query_xyz, support_xyz, 1) and idx.is_cuda:
            return knn_group_dp(idx.int().contiguous(), query_xyz.detach().contiguous(), support_xyz.detach().contiguous(),
                                self.relative_xyz, self.normalize_dp)
        grouped_xyz = torch_grouping_operation(support_xyz.transpose(1, 2).contiguous(), idx)
        if self.relative_xyz:
            grouped_xyz -= query_xyz.transpose(1, 2).unsqueeze(-1)
        if self.normalize_dp:
            grouped_xyz /= torch.amax(torch.sqrt(torch.sum(grouped_xyz**2, dim=1)), dim=(1, 2)).view(-1, 1, 1, 1)
        return grouped_xyz

    def forward(self, query_xyz, support_xyz, features=None, geom=None):
        """query (B,npoint,3), support (B,N,3), features (B,C,N)
        -> relative positions (B,3,npoint,nsample), grouped features (B,C,npoint,nsample) or None"""
        idx = geom['idx'] if geom is not None else self.query(query_xyz, support_xyz)
        if self.return_only_idx:
            return idx
        grouped_xyz = geom['dp'] if geom is not None else self.relative_positions(idx, query_xyz, support_xyz)
        if features is None:
            return grouped_xyz, None
        group = grouping_operation if features.is_cuda else torch_grouping_operation
        return grouped_xyz, group(features, idx)


class GroupAll(nn.Module):
    def forward(self, new_xyz, xyz, features=None, geom=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        grouped_features = features.unsqueeze(2) if features is not None else None
        return grouped_xyz, grouped_features


def get_aggregation_feautres(p, dp, f, fj, feature_type='dp_fj'):
    if feature_type == 'dp_fj':
        return torch.cat([dp, fj], 1)
    if feature_type == 'dp_fj_df':
        return torch.cat([dp, fj, fj - f.unsqueeze(-1)], 1)
    if feature_type == 'pi_dp_fj_df':
        df = fj - f.unsqueeze(-1)
        pi = p.transpose(1, 2).unsqueeze(-1).expand(-1, -1, -1, df.shape[-1])
        return torch.cat([pi, dp, fj, df], 1)
    if feature_type == 'dp_df':
        return torch.cat([dp, fj - f.unsqueeze(-1)], 1)
    return fj


def create_grouper(group_args):
    args = copy.deepcopy(group_args)
    method = args.pop('NAME', 'ballquery')
    radius = args.pop('radius', 0.1)
    nsample = args.pop('nsample', 20)
    logging.info(group_args)
    if nsample is None:
        return GroupAll()
    if method == 'ballquery':
        return QueryAndGroup(radius, nsample, **args)
    if method == 'knn':
        return KNNGroup(nsample, **args)
    raise NotImplementedError(f"grouper {method!r}: 'ballquery' and 'knn' are the reference's groupers")
