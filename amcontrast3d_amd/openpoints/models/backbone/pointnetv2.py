"""PointNet++ (single- and multi-scale grouping) and ASSANet backbones on the gfx950 kernels.

API mirror of models/backbone/pointnetv2.py: ``PointNetSAModuleMSG`` (:18-100), ``PointNetFPModule`` (:103-146),
``PointNet2Encoder`` (:149-344), ``PointNet2Decoder`` (:347-380) and ``PointNet2PartDecoder`` (:383-511), the last three in the
``MODELS`` registry, with the reference's constructor arguments, channel arithmetic, attribute names and module nesting
(state-dict keys).  ASSANet is the same encoder with ``aggr_args.NAME: 'ASSA'``, ``stem_conv``, ``stem_aggr``,
``query_as_support``, ``use_res`` and ``double_last_channel: False``.

Geometry / feature split as in the PointNeXt blocks: every module has a coordinate-only ``plan*`` method and a forward that
consumes the plan (``geom``) or builds it.  ``PointNet2Encoder.plan_geometry(p0)`` returns the stem's plan and, per SA module,
the FPS picks, the sub-sampled cloud and one plan per scale; ``forward_seg_feat`` reads it from
``data['_geometry']['encoder']`` when the batch carries it, and ``BaseSeg`` hands ``data['_geometry']['decoder']``
(``PointNet2Decoder.plan_geometry``) to the decoder.
"""
import logging
from typing import List, Optional

import torch
import torch.nn as nn

from amcontrast3d_amd.geometry import plan_key
from ..build import MODELS
from ..layers import (LocalAggregation, create_convblock1d, expand_cloud_channels, feature_propagation_first_block,
                      furthest_point_sample, random_sample, run_convblocks, three_interpolate)


class PointNetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping: sub-sample the support cloud once, then aggregate around the samples
    once per scale (radius, nsample, MLP) and concatenate.  With ``query_as_support`` the scales form a chain instead: the
    output of one is the support of the next, on the sampled cloud (ASSANet's blocks)."""

    def __init__(self, stride: int, radii: List[float], nsamples: List[int], channel_list: List[List[int]], aggr_args: dict,
                 group_args: dict, conv_args: dict, norm_args: dict, act_args: dict, sampler='fps', use_res=False,
                 query_as_support=False, voxel_size=0.1, **kwargs):
        super().__init__()
        self.stride = stride
        self.blocks = len(channel_list)
        self.query_as_support = query_as_support
        name = sampler.lower()
        if 'fps' in name or 'furthest' in name:
            self.sample_fn = furthest_point_sample
        elif 'random' in name:
            self.sample_fn = random_sample
        self.local_aggregations = nn.ModuleList()
        for i, (radius, nsample) in enumerate(zip(radii, nsamples)):
            channels = channel_list[i]
            if i > 0 and query_as_support:
                channels[0] = channel_list[i - 1][-1]
            group_args.radius = radius  # written into the caller's config, as the reference does
            group_args.nsample = nsample
            self.local_aggregations.append(
                LocalAggregation(channels, aggr_args, conv_args, norm_args, act_args, group_args, use_res))

    @torch.no_grad()
    def plan_sample(self, support_xyz):
        """FPS picks and the sub-sampled cloud (the serial part of the geometry)"""
        if self.stride > 1:
            idx = self.sample_fn(support_xyz, support_xyz.shape[1] // self.stride).long()
            return {'fps_idx': idx, 'new_p': torch.gather(support_xyz, 1, idx.unsqueeze(-1).expand(-1, -1, 3))}
        return {'fps_idx': None, 'new_p': support_xyz}

    @torch.no_grad()
    def plan_group(self, support_xyz, g):
        """one plan per scale (in place into g['blocks']).  With query_as_support the scales after the first are self queries
        of the sampled cloud and share a plan per (grouper class, radius, nsample) among operators of one class, depth,
        feature recipe and reduction (they decide which moments and lists a plan carries)."""
        query_xyz, cache, blocks = g['new_p'], {}, []
        for i, la in enumerate(self.local_aggregations):
            if self.query_as_support and i > 0:
                op = la.SA_CONFIG_operator  # what a plan holds also depends on the operator: its class, depth and recipe
                key = plan_key(op.grouper) + (type(op), len(op.convs), op.feature_type, op.reduction)
                if key not in cache:
                    cache[key] = la.plan(query_xyz, query_xyz)
                blocks.append(cache[key])
            else:
                blocks.append(la.plan(query_xyz, support_xyz))
        g['blocks'] = blocks
        return g

    def plan(self, support_xyz):
        return self.plan_group(support_xyz, self.plan_sample(support_xyz))

    def forward(self, support_xyz, support_features=None, query_xyz=None, geom=None):
        """support_xyz (B,N,3), support_features (B,C,N) -> the sampled cloud (B,N/stride,3) and the concatenated
        features of all scales (B, sum of the last widths, N/stride).  As in the reference a `query_xyz` handed in is not
        used: the module samples when its stride is above 1 and queries around every support point otherwise."""
        if query_xyz is None and self.stride > 1:
            if geom is None:
                geom = self.plan(support_xyz)
            idx, query_xyz = geom['fps_idx'], geom['new_p']
        else:
            if geom is None:
                geom = self.plan_group(support_xyz, {'fps_idx': None, 'new_p': support_xyz})
            idx, query_xyz = None, support_xyz
        outs = []
        for i in range(self.blocks):
            f = self.local_aggregations[i](query_xyz, support_xyz, support_features, query_idx=idx, geom=geom['blocks'][i])
            outs.append(f)
            if self.query_as_support:
                support_xyz, support_features, idx = query_xyz, f, None
        return query_xyz, torch.cat(outs, dim=1)


class PointNetFPModule(nn.Module):
    """Feature propagation: 3-NN inverse-distance interpolation of the known (coarse) features onto the unknown (fine)
    cloud, concatenation with the fine cloud's own features, point-wise MLP."""

    def __init__(self, mlp: List[int], norm_args={'norm': 'bn1d'}, act_args={'act': 'relu'}):
        super().__init__()
        self.convs = nn.Sequential(*[create_convblock1d(mlp[i], mlp[i + 1], norm_args=norm_args, act_args=act_args)
                                     for i in range(len(mlp) - 1)])

    @staticmethod
    @torch.no_grad()
    def plan(unknown, known):
        """coordinate-only part: the 3 nearest known points of every unknown point and their inverse-distance weights"""
        from .pointnext_blocks import FeaturePropogation
        return FeaturePropogation.plan(unknown, known)

    def forward(self, unknown, known, unknow_feats, known_feats, geom=None, cloud=None):
        """`cloud`: e (B,E), channels constant along a cloud's points that the reference concatenates in front of
        unknow_feats (PointNet2PartDecoder's one-hot shape category): a per-cloud term of the first conv where the block has
        the form for it (cloud_term_route), expanded and concatenated otherwise."""
        if cloud is not None:
            if known is not None and len(self.convs) and unknow_feats is not None:
                if geom is None:
                    geom = self.plan(unknown, known)
                first = feature_propagation_first_block(self.convs[0], unknow_feats, known_feats, geom, (cloud, cloud.shape[1]))
                if first is not None:
                    return run_convblocks(list(self.convs)[1:], first)
            unknow_feats = expand_cloud_channels(cloud, unknow_feats)
        if known is None:
            up = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        else:
            if geom is None:
                geom = self.plan(unknown, known)
            first = (feature_propagation_first_block(self.convs[0], unknow_feats, known_feats, geom)
                     if len(self.convs) and unknow_feats is not None else None)
            if first is not None:  # the first conv on both branches before the interpolation: no concatenated tensor
                return run_convblocks(list(self.convs)[1:], first)
            up = three_interpolate(known_feats, geom['idx'], geom['weight'], geom.get('csr'))
        return run_convblocks(self.convs, up if unknow_feats is None else torch.cat([unknow_feats, up], dim=1))


@MODELS.register_module()
class PointNet2Encoder(nn.Module):
    """Encoder of PointNet++ and ASSANet.

    radius / num_samples: a scalar (scaled per stage by radius_scaling / nsample_scaling, per later block by
    block_radius_scaling) or a list per stage (a scalar or a list per block).  mlps: the widths per stage and block, or None
    with width / layers / blocks (double_last_channel: the last layer of a stage's first block doubles the width).
    use_res, stem_conv, stem_aggr, query_as_support and double_last_channel=False are ASSANet's settings."""

    def __init__(self, in_channels: int, radius, num_samples, aggr_args: dict, group_args: dict, conv_args: dict,
                 norm_args: dict, act_args: dict, blocks: Optional[List] = None, mlps=None, width: Optional[int] = None,
                 strides: List[int] = [4, 4, 4, 4], layers: int = 3, width_scaling: int = 2, radius_scaling: int = 2,
                 block_radius_scaling: int = 1, nsample_scaling: int = 1, sampler: str = 'fps', use_res=False, stem_conv=False,
                 stem_aggr=False, double_last_channel=True, query_as_support=False, **kwargs):
        super().__init__()
        if kwargs:
            logging.warning(f"kwargs: {kwargs} are not used in {__class__.__name__}")
        stages = len(strides)
        self.strides = strides
        self.blocks = blocks if mlps is None else [len(mlp) for mlp in mlps]
        radius = self._to_full_list(radius, blocks=self.blocks, param_scaling=radius_scaling,
                                    block_param_scaling=block_radius_scaling)
        num_samples = self._to_full_list(num_samples, blocks=self.blocks, param_scaling=nsample_scaling)
        self.radius = radius
        self.num_samples = num_samples
        logging.info(f'radius is modified to {radius}')
        logging.info(f'num_samples is modified to {num_samples}')

        self.stem_conv = stem_conv
        self.stem_aggr = stem_aggr
        if stem_conv:
            width = width if width is not None else mlps[0][0][0]
            self.conv1 = create_convblock1d(in_channels, width, norm_args=None, act_args=None)
            if stem_aggr:
                group_args.radius = radius[0][0]
                group_args.nsample = num_samples[0][0]
                self.stem = LocalAggregation([width] * (layers + 1), aggr_args, conv_args, norm_args, act_args, group_args,
                                             use_res)
            in_channels = width

        if mlps is None:
            assert width is not None
            assert layers is not None
            assert strides is not None
            mlps = []
            for i in range(stages):
                if not double_last_channel:
                    mlps.append([[width] * layers] * self.blocks[i])  # (the blocks of a stage share ONE list object)
                    width = width * width_scaling if strides[i] > 1 else width
                else:
                    first = [width] * (layers - 1)
                    width = width * width_scaling if strides[i] > 1 else width
                    first += [width]
                    mlps.append([first] + [[width] * layers] * (self.blocks[i] - 1))
            logging.info(f'channels is modified to {mlps}')
        self.mlps = mlps

        self.SA_modules = nn.ModuleList()
        skip_channel_list = [in_channels]
        for k in range(stages):
            channel_list = mlps[k].copy()
            channel_out = 0
            for j in range(len(channel_list)):
                channel_list[j] = [in_channels] + channel_list[j]
                channel_out += channel_list[j][-1]  # the scales are concatenated
            self.SA_modules.append(PointNetSAModuleMSG(
                stride=strides[k], radii=radius[k], nsamples=num_samples[k], channel_list=channel_list, aggr_args=aggr_args,
                group_args=group_args, conv_args=conv_args, norm_args=norm_args, act_args=act_args, sampler=sampler,
                use_res=use_res, query_as_support=query_as_support))
            skip_channel_list.append(channel_out)
            in_channels = channel_out
        self.out_channels = channel_out
        self.channel_list = skip_channel_list

    def _to_full_list(self, param, blocks, param_scaling=1, block_param_scaling=1):
        """radius / nsample as one value per stage and block"""
        full = []
        if isinstance(param, List):
            for i, value in enumerate(param):
                value = [value] if not isinstance(value, List) else value
                if len(value) != blocks[i]:
                    value += [value[-1]] * (blocks[i] - len(value))
                full.append(value)
        else:
            for i, stride in enumerate(self.strides):
                if stride == 1:
                    full.append([param] * blocks[i])
                else:
                    full.append([param] + [param * block_param_scaling] * (blocks[i] - 1))
                    param *= param_scaling
        return full

    @torch.no_grad()
    def plan_geometry(self, p0):
        """Coordinate-only half of the encoder: {'stem': the stem aggregation's plan or None, 'modules': per SA module
        {'fps_idx', 'new_p', 'blocks': one plan per scale}}; the clouds of all levels are p0 and every module's 'new_p'."""
        p0 = p0.contiguous()
        stem = self.stem.plan(p0, p0) if self.stem_aggr and self.stem_conv else None
        modules, p = [], p0
        for sa in self.SA_modules:
            g = sa.plan(p)
            modules.append(g)
            p = g['new_p']
        return {'stem': stem, 'modules': modules}

    def _split(self, xyz, features):
        geom = None
        if hasattr(xyz, 'keys'):
            data = xyz
            xyz, features = data['pos'], data['x']
            plan = data.get('_geometry', None)
            geom = plan.get('encoder') if plan is not None else None
        if features is None:
            features = xyz.clone().transpose(1, 2).contiguous()
        return xyz, features, geom

    def forward_cls_feat(self, xyz, features=None):
        xyz, features, geom = self._split(xyz, features)
        if self.stem_conv:
            features = run_convblocks((self.conv1,), features)
        if self.stem_aggr:
            features = self.stem(xyz, xyz, features, geom=None if geom is None else geom['stem'])
        for i, sa in enumerate(self.SA_modules):
            xyz, features = sa(xyz, features, geom=None if geom is None else geom['modules'][i])
        return features.squeeze(-1)

    def forward_seg_feat(self, xyz, features=None):
        xyz, features, geom = self._split(xyz, features)
        xyz = xyz.contiguous()
        if self.stem_conv:
            features = run_convblocks((self.conv1,), features)
        if self.stem_aggr:
            features = self.stem(xyz, xyz, features, geom=None if geom is None else geom['stem'])
        l_xyz, l_features = [xyz], [features]
        for i, sa in enumerate(self.SA_modules):
            li_xyz, li_features = sa(l_xyz[i], l_features[i], geom=None if geom is None else geom['modules'][i])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        return l_xyz, l_features

    def forward(self, xyz, features=None):
        return self.forward_seg_feat(xyz, features)


@MODELS.register_module()
class PointNet2Decoder(nn.Module):
    """Decoder of PointNet++: one feature-propagation module per encoder level, coarse to fine."""

    def __init__(self, encoder_channel_list: List[int], mlps=None, fp_mlps=None, decoder_layers=1, **kwargs):
        super().__init__()
        skip_channel_list = encoder_channel_list
        self.FP_modules = nn.ModuleList()
        if fp_mlps is None:
            fp_mlps = [[mlps[0][0][0]] * (decoder_layers + 1)]
            fp_mlps += [[c] * (decoder_layers + 1) for c in skip_channel_list[1:-1]]
        for k in range(len(fp_mlps)):
            pre_channel = fp_mlps[k + 1][-1] if k + 1 < len(fp_mlps) else skip_channel_list[-1]
            self.FP_modules.append(PointNetFPModule([pre_channel + skip_channel_list[k]] + fp_mlps[k]))
        self.out_channels = fp_mlps[0][-1]

    @torch.no_grad()
    def plan_geometry(self, l_xyz):
        """3-NN indices / weights of every level: entry i serves FP_modules[i] (fine cloud l_xyz[i], coarse l_xyz[i + 1])"""
        return [PointNetFPModule.plan(l_xyz[i], l_xyz[i + 1]) for i in range(len(self.FP_modules))]

    def forward(self, l_xyz, l_features, geom=None):
        n = len(self.FP_modules)
        for i in range(-1, -(n + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i],
                                                   geom=None if geom is None else geom[n + i])
        return l_features[0]


def shape_one_hot(cls_label, num_classes, device):
    """(B, num_classes) fp32 one-hot rows of the shape categories cls_label (B,1) (or (B,)) int64"""
    one_hot = torch.zeros((cls_label.shape[0], num_classes), device=device)
    return one_hot.scatter_(1, cls_label.reshape(-1, 1).to(device), 1)


@MODELS.register_module()
class PointNet2PartDecoder(nn.Module):
    """Part-segmentation decoder of PointNet++ (pointnetv2.py:383-511): PointNet2Decoder's feature propagation, with the
    16-way one-hot of the shape category in front of the input features at the finest level.  It is built from the encoder's
    constructor arguments and repeats its channel arithmetic (as there: double_last_channel defaults to False, and without
    it the width is scaled BEFORE a stage's list is made).  The one-hot channels are constant along a cloud: FP_modules[0]
    takes them as a per-cloud term of its first conv (PointNetFPModule.forward, `cloud`)."""

    def __init__(self, in_channels: int, radius, num_samples, group_args: dict, conv_args: dict, norm_args: dict, act_args: dict,
                 mlps=None, blocks: Optional[List] = None, width: Optional[int] = None, strides=[4, 4, 4, 4], layers=3,
                 fp_mlps=None, decoder_layers=1, decocder_aggr_args=None, width_scaling=2, radius_scaling=2, nsample_scaling=1,
                 use_res=False, stem_conv=False, double_last_channel=False, **kwargs):
        super().__init__()
        if kwargs:
            logging.warning(f"kwargs: {kwargs} are not used in {__class__.__name__}")
        stages = len(strides)
        self.strides = strides
        self.blocks = blocks if mlps is None else [len(mlp) for mlp in mlps]
        self.radius = self._to_full_list(radius, self.blocks, param_scaling=radius_scaling)
        self.num_samples = self._to_full_list(num_samples, self.blocks, param_scaling=nsample_scaling)
        if stem_conv:
            in_channels = width
        if mlps is None:
            assert width is not None
            assert layers is not None
            assert strides is not None
            mlps = []
            for i in range(stages):
                if not double_last_channel:
                    width = width * width_scaling if strides[i] > 1 else width
                    mlps.append([[width] * layers] * self.blocks[i])
                else:
                    first = [width] * (layers - 1)
                    width = width * 2 if strides[i] > 1 else width
                    first += [width]
                    mlps.append([first] + [[width] * layers] * (self.blocks[i] - 1))
            logging.info(f'channels is modified to {mlps}')
        self.mlps = mlps

        skip_channel_list = [in_channels]
        for k in range(stages):
            channel_out = sum(mlp[-1] for mlp in mlps[k])  # the scales are concatenated
            skip_channel_list.append(channel_out)
            in_channels = channel_out

        self.FP_modules = nn.ModuleList()
        if fp_mlps is None:
            fp_mlps = [[mlps[0][0][0]] * (decoder_layers + 1)]
            fp_mlps += [[c] * (decoder_layers + 1) for c in skip_channel_list[1:-1]]
        self.num_shape_classes = 16
        skip_channel_list[0] += self.num_shape_classes
        for k in range(len(fp_mlps)):
            pre_channel = fp_mlps[k + 1][-1] if k + 1 < len(fp_mlps) else skip_channel_list[-1]
            self.FP_modules.append(PointNetFPModule([pre_channel + skip_channel_list[k]] + fp_mlps[k]))
        self.out_channels = fp_mlps[0][-1]

    _to_full_list = PointNet2Encoder._to_full_list  # reads self.strides only; pads the caller's lists in place as there

    @torch.no_grad()
    def plan_geometry(self, l_xyz):
        """3-NN indices / weights of every level: entry i serves FP_modules[i] (fine cloud l_xyz[i], coarse l_xyz[i + 1])"""
        return [PointNetFPModule.plan(l_xyz[i], l_xyz[i + 1]) for i in range(len(self.FP_modules))]

    def forward(self, l_xyz, l_features, cls_label, geom=None):
        n = len(self.FP_modules)
        for i in range(-1, -n, -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i],
                                                   geom=None if geom is None else geom[n + i])
        one_hot = shape_one_hot(cls_label, self.num_shape_classes, l_xyz[0].device)
        l_features[0] = self.FP_modules[0](l_xyz[0], l_xyz[1], l_features[0], l_features[1],
                                           geom=None if geom is None else geom[0], cloud=one_hot)
        return l_features[0]
