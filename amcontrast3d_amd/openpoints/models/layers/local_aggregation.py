"""Local aggregation operators of PointNet++ and ASSANet on the gfx950 kernels.

API mirror of models/layers/local_aggregation.py -- ``ConvPool`` (:141-242, the grouped MLP + pooling of PointNet++),
``ASSA`` (:32-138, the separable set abstraction of ASSANet) and the ``LocalAggregation`` wrapper (:246-286) that picks one
by ``aggr_args.NAME`` -- with the reference's constructor arguments, defaults, attribute names and module nesting, hence
its state-dict keys (``SA_CONFIG_operator.convs.{i}.{0,1}.*``, ``.skipconv.0.*``, ``.skip_layer.*``).  The constructors
edit the caller's ``channels`` list in place as the reference's do.  backbone/pointnext_blocks.py::LocalAggregation is a
different class (PointNeXt's).

Both operators follow the plan protocol of the PointNeXt blocks: ``plan(query_xyz, support_xyz)`` is the coordinate-only
half (neighbour indices, relative positions, and the moments / reverse lists a kernel route needs), ``forward`` consumes
such a plan (``geom``) and builds it itself when none is handed in.

Routes.  ConvPool with 'dp_fj' features, max pooling and fp32 GPU features convolves before it gathers, exactly as
SetAbstraction.forward does: one conv block -> fused_local_aggregation; several with 32 neighbours -> fused_first_block
and run_convblocks on the activated first layer (a two-block rest -- PointNet++ stacks three convs -- runs conv, BatchNorm,
conv and the BatchNorm + max kernel one after another: the recomputing tail of csrc/sa_tail.hip covers a one-block rest
only); otherwise the fused gather + first conv (fused_first_conv) where its widths allow.  Everything else is the
reference's composition (group, concatenate, run_convblocks, pool).  ConvPool's 1x1 convs always run on this library's own
kernels (run_convblocks(library=False)): a max over the neighbours follows them, and the convolution library's choice of
kernel, made per session, would flip arg-maxes from one session to the next.  ASSA runs its pre- and post-convolutions through
run_convblocks and the aggregation between them as ops.SeparableAggregation (csrc/assa.hip).
"""
from typing import List

import numpy as np
import torch
import torch.nn as nn

from amcontrast3d_amd import ops
from .blocks import (CHANNEL_MAP, _eval_bn, _fusable_bn, _grouped_first_block, _synced_bn_group, conv1x1, conv_bn_block,
                     create_act, create_convblock1d, create_convblock2d, fused_first_block, fused_first_conv,
                     fused_local_aggregation, run_convblocks)
from .group import create_grouper, get_aggregation_feautres


def _reduction_layer(reduction):
    if reduction == 'max':
        return lambda x: torch.max(x, dim=-1, keepdim=False)[0]
    if reduction in ('avg', 'mean'):
        return lambda x: torch.mean(x, dim=-1, keepdim=False)
    if reduction == 'sum':
        return lambda x: torch.sum(x, dim=-1, keepdim=False)
    raise NotImplementedError(f'reduction {reduction} not implemented')


@torch.no_grad()
def _plan(grouper, query_xyz, support_xyz, convs=None, feature_type=None, lists=False):
    """idx and dp of one query; for a ConvPool stack whose route reads them (`convs`) the moments / reverse lists of the
    convolve-before-gather kernels, for ASSA (`lists`) the reverse lists its deterministic backward gathers over"""
    if not hasattr(grouper, 'query'):  # GroupAll: nothing to search
        return None
    idx = grouper.query(query_xyz, support_xyz)
    dp = grouper.relative_positions(idx, query_xyz, support_xyz)
    g = {'idx': idx, 'dp': dp}
    n = support_xyz.shape[1]
    if convs is not None:
        from ..backbone.pointnext_blocks import _csr, _moments
        g['csr'] = _csr(convs, feature_type, idx, n, dp)
        g['mom'] = _moments(convs, feature_type, idx, dp, n, g['csr'])
    elif lists and idx.is_cuda:
        start, edge = ops.group_csr(idx, n)
        g['csr'] = {'start': start, 'edge': edge}
    return g


class ASSA(nn.Module):
    """Point-wise convs on the support points, anisotropic separable aggregation over the neighbourhood (every neighbour
    feature times each coordinate of its relative position, reduced over the neighbours), point-wise convs on the result,
    and a residual from the pre-convolved features."""

    def __init__(self, channels: List[int], conv_args=None, norm_args=None, act_args=None, group_args=None,
                 feature_type='dp_fj', reduction='mean', use_res=True, use_inverted_dims=False):
        super(ASSA, self).__init__()
        self.feature_type = feature_type
        self.use_res = use_res
        n_layers = len(channels) - 1
        num_preconv = int(np.ceil(n_layers / 2))
        self.num_preconv = num_preconv
        if feature_type == 'assa' and not use_inverted_dims:  # the x3 of the aggregation restores the width
            channels[num_preconv] = int(np.ceil(channels[num_preconv] / 3.0))
        convs = [create_convblock1d(channels[i], channels[i + 1], norm_args=norm_args, act_args=act_args, **conv_args)
                 for i in range(num_preconv)]
        skip_channels = channels[num_preconv]
        channels[num_preconv] = CHANNEL_MAP[feature_type](channels[num_preconv])
        for i in range(num_preconv, n_layers):
            last_of_residual = use_res and i == n_layers - 1
            convs.append(create_convblock1d(channels[i], channels[i + 1], norm_args=norm_args,
                                            act_args=None if last_of_residual else act_args, **conv_args))
        self.act = create_act(act_args)
        self.convs = nn.Sequential(*convs)
        if use_res:
            self.skip_layer = (nn.Identity() if skip_channels == channels[-1]
                               else nn.Conv1d(skip_channels, channels[-1], 1, bias=False))
        self.grouper = create_grouper(group_args)
        self.reduction = reduction
        self.reduction_layer = _reduction_layer(reduction)

    def plan(self, query_xyz, support_xyz):
        """coordinate-only part: neighbour indices, relative positions and, in deterministic mode, the reverse lists"""
        return _plan(self.grouper, query_xyz, support_xyz, lists=ops.deterministic())

    def forward(self, query_xyz, support_xyz, features, query_idx=None, geom=None):
        mods = list(self.convs)
        features = run_convblocks(mods[:self.num_preconv], features)
        if geom is None:
            geom = self.plan(query_xyz, support_xyz)
        if geom is None:
            raise NotImplementedError("ASSA needs a grouper with neighbour indices (ballquery or knn)")
        csr = geom.get('csr')
        out = ops.separable_aggregation(features, geom['idx'], geom['dp'], self.reduction,
                                        (csr['start'], csr['edge']) if csr is not None else None)
        if not self.use_res:
            return run_convblocks(mods[self.num_preconv:], out)
        if query_idx is not None:
            features = torch.gather(features, -1, query_idx.unsqueeze(1).expand(-1, features.shape[1], -1))
        skip = features if isinstance(self.skip_layer, nn.Identity) else conv1x1(self.skip_layer, features)
        if type(self.act) is nn.ReLU:  # relu(. + skip) inside the last BatchNorm's kernels where the block has that form
            return run_convblocks(mods[self.num_preconv:], out, residual=skip)
        return self.act(run_convblocks(mods[self.num_preconv:], out) + skip)


class ConvPool(nn.Module):
    """Shared MLP over [relative position ; neighbour features ...] of every neighbourhood, then pooling."""

    def __init__(self, channels: List[int], conv_args=None, norm_args=None, act_args=None, group_args=None,
                 feature_type='dp_fj', reduction='mean', use_res=False, use_pooled_as_identity=False, **kwargs):
        super(ConvPool, self).__init__()
        skip_channel = channels[0]
        self.use_res = use_res
        self.use_pooled_as_identity = use_pooled_as_identity
        if use_res:
            self.skipconv = (create_convblock1d(skip_channel, channels[-1], norm_args=None, act_args=None, **conv_args)
                             if skip_channel != channels[-1] else nn.Identity())
        self.feature_type = feature_type
        channels[0] = CHANNEL_MAP[feature_type](channels[0])
        n_layers = len(channels) - 1
        convs = [create_convblock2d(channels[i], channels[i + 1], norm_args=norm_args,
                                    act_args=None if (use_res and i == n_layers - 1) else act_args, **conv_args)
                 for i in range(n_layers)]
        self.act = create_act(act_args)
        self.convs = nn.Sequential(*convs)
        self.grouper = create_grouper(group_args)
        self.reduction = reduction
        self.reduction_layer = _reduction_layer(reduction)

    def _moments_route(self, nsample):
        """'pooled' / 'first_block' when the stack has the form and widths of the route that reads the plan's moments and
        reverse lists (module inspection only: features and mode are forward's), else None"""
        if self.feature_type != 'dp_fj' or self.reduction != 'max' or nsample is None:
            return None
        m = conv_bn_block(self.convs[0])
        if m is None or m[0].bias is not None:
            return None
        cout = m[0].out_channels
        if len(self.convs) == 1:
            return 'pooled' if ops.local_aggregation_supported(cout, nsample) else None
        return 'first_block' if m[2] is not None and ops.grouped_conv_bn_supported(cout, nsample) else None

    def plan(self, query_xyz, support_xyz):
        """coordinate-only part: neighbour indices and relative positions; moments and reverse lists only for a stack whose
        route reads them ('pooled', 'first_block'): 'first_conv' and the composition need idx and dp alone"""
        extras = self._moments_route(getattr(self.grouper, 'nsample', None)) is not None
        return _plan(self.grouper, query_xyz, support_xyz, self.convs if extras else None, self.feature_type)

    def route(self, f, geom):
        """which of the routes of the module docstring forward takes for these features and this plan -- 'pooled' (one launch
        family for conv + BatchNorm + max), 'first_block', 'first_conv' or 'composition' -- from the same conditions the fused
        layers check; nothing is launched and no state changes"""
        if self.reduction != 'max' or geom is None:
            return 'composition'
        m = _grouped_first_block(self.convs, f, geom, self.feature_type)
        if m is None:
            return 'composition'
        conv, bn, _ = m
        name = self._moments_route(geom['idx'].shape[-1])
        if (name is not None and geom.get('mom') is not None
                and (_eval_bn(bn, f) or _synced_bn_group(bn, f) is not None or _fusable_bn(bn, f))):
            return name
        return 'first_conv' if ops.grouped_conv_supported(f.shape[1], conv.out_channels) else 'composition'

    def forward(self, query_xyz, support_xyz, features, query_idx=None, geom=None):
        if geom is None:
            geom = self.plan(query_xyz, support_xyz)
        support_features = features
        identity, neighbor_dim = 0, 3
        fj = None
        if 'df' in self.feature_type or self.use_res:
            if self.use_pooled_as_identity:
                dp, fj = self.grouper(query_xyz, support_xyz, support_features, geom=geom)
                features = torch.max(fj, dim=-1, keepdim=False)[0]
            elif query_idx is not None:
                if query_xyz.shape[1] != support_xyz.shape[1]:
                    features = torch.gather(features, -1, query_idx.unsqueeze(1).expand(-1, features.shape[1], -1))
            elif geom is None or geom['dp'].shape[2] == 1:
                neighbor_dim = 2  # one query (GroupAll has no plan): the layer aggregates the whole cloud
            if self.use_res and neighbor_dim != 2:
                identity = run_convblocks((self.skipconv,), features, library=False)
        route, out = self.route(support_features, geom), None
        if route == 'pooled':
            out = fused_local_aggregation(self.convs, support_features, geom, self.feature_type)
        elif route == 'first_block':
            x1 = fused_first_block(self.convs, support_features, geom, self.feature_type)
            if x1 is not None:
                out = run_convblocks(list(self.convs)[1:], x1, pool_max=True, activated=True, library=False)
        elif route == 'first_conv':
            pre = fused_first_conv(self.convs, support_features, geom, self.feature_type)
            if pre is not None:
                out = run_convblocks(self.convs, None, pool_max=True, pre=pre, library=False)
        if out is None:
            if route != 'composition':
                raise RuntimeError(f"ConvPool: route {route!r} was chosen and its layer declined")
            if fj is None:
                dp, fj = self.grouper(query_xyz, support_xyz, support_features, geom=geom)
            fj = get_aggregation_feautres(query_xyz, dp, features, fj, feature_type=self.feature_type)
            if self.reduction == 'max':
                out = run_convblocks(self.convs, fj, pool_max=True, library=False)
            else:
                out = self.reduction_layer(run_convblocks(self.convs, fj, library=False))
        if self.use_res:
            out = self.act(out + identity)
        return out


class LocalAggregation(nn.Module):
    """One local aggregation = one residual block of the backbone: ConvPool or ASSA by ``aggr_args.NAME``."""

    def __init__(self, channels: List[int], aggr_args: dict, conv_args=None, norm_args=None, act_args=None, group_args=None,
                 use_res=False):
        super(LocalAggregation, self).__init__()
        aggr_type = aggr_args.get('NAME', 'convpool')
        feature_type = aggr_args.get('feature_type', 'dp_fj')
        reduction = aggr_args.get('reduction', 'max')
        use_inverted_dims = aggr_args.get('use_inverted_dims', False)
        use_pooled_as_identity = aggr_args.get('use_pooled_as_identity', False)
        if aggr_type.lower() == 'convpool':
            self.SA_CONFIG_operator = ConvPool(channels, conv_args, norm_args, act_args, group_args, feature_type, reduction,
                                               use_res, use_pooled_as_identity)
        elif aggr_type.lower() == 'assa':
            self.SA_CONFIG_operator = ASSA(channels, conv_args, norm_args, act_args, group_args, feature_type, reduction,
                                           use_res, use_inverted_dims)
        else:
            raise NotImplementedError(f'LocalAggregation {aggr_type.lower()} not implemented')

    def plan(self, query_xyz, support_xyz):
        return self.SA_CONFIG_operator.plan(query_xyz, support_xyz)

    def forward(self, query_xyz, support_xyz, support_features, query_idx=None, geom=None):
        return self.SA_CONFIG_operator(query_xyz, support_xyz, support_features, query_idx, geom=geom)
