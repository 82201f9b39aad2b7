"""The plain PointNeXt encoder / decoder: the baseline AMContrast3D is compared against.

Drop-in for openpoints/models/backbone/pointnext.py: same registered class names, constructor keywords, attribute
names and module nesting (hence state-dict keys -- which are also those of the _AMContrast3D classes):

    PointNextEncoder      pointnext.py:310-458
    PointNextDecoder      :461-498
    PointNextPartDecoder  :501-665

The modules are those of pointnext_AA.py (the reference's two files define the same blocks twice); what differs is the
forward: (p, f) lists only, no stageACE_list and no per-stage rows for a contrastive loss.  The coordinate-only half
(``'_geometry'`` in the batch dict, amcontrast3d_amd/geometry.py) is consumed as there and built in line when absent.
"""
from typing import List

import torch
import torch.nn as nn

from amcontrast3d_amd.geometry import plan_key

from ..build import MODELS
from ..layers import create_convblock1d, run_convblocks
from .pointnetv2 import shape_one_hot
from .pointnext_AA import PointNextDecoder_AMContrast3D, PointNextEncoder_AMContrast3D
from .pointnext_blocks import _BLOCKS, FeaturePropogation


@MODELS.register_module()
class PointNextEncoder(PointNextEncoder_AMContrast3D):
    def forward_seg_feat(self, p0, f0=None, geometry=None):
        """-> p[6], f[6] (pointnext.py:443-455).  `geometry`: the plan's 'encoder' entry, when p0 is not a batch dict
        that carries one."""
        if hasattr(p0, 'keys'):
            if geometry is None and p0.get('_geometry', None) is not None:
                geometry = p0['_geometry']['encoder']
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        if geometry is None:
            geometry = self.plan_geometry(p0)
        p, f = [p0], [f0]
        for stage, plans in zip(self.encoder, geometry):
            pf = [p[-1], f[-1]]
            for blk, g in zip(stage, plans):
                pf = blk(pf, geom=g)
            p.append(pf[0])
            f.append(pf[1])
        return p, f

    def forward(self, p0, f0=None):
        return self.forward_seg_feat(p0, f0)


@MODELS.register_module()
class PointNextDecoder(PointNextDecoder_AMContrast3D):
    def forward(self, p, f, geometry=None):
        """-> the finest level's features (pointnext.py:494-498).  `geometry`: the plan's 'decoder' entry."""
        if geometry is None:
            geometry = self.plan_geometry(p)
        for i in range(-1, -len(self.decoder) - 1, -1):
            f[i - 1] = self.decoder[i][1:](
                [p[i], self.decoder[i][0]([p[i - 1], f[i - 1]], [p[i], f[i]], geom=geometry[i])])[1]
        return f[-len(self.decoder) - 1]


@MODELS.register_module()
class PointNextPartDecoder(nn.Module):
    """Part-segmentation decoder of PointNeXt (pointnext.py:501-665): feature propagation per level, optionally followed by
    InvResMLP blocks on the level's fine cloud (decoder_blocks > 1), with the shape category entering the finest level as
    extra input channels in front of the skip features.  `cls_map` chooses what those channels are:

        'pointnet2'   ReLU(convc(16-way one-hot))                                   64 channels
        'curvenet'    [max global_conv1(f[-2]) ; max global_conv2(f[-1]) ; one-hot]  64 + 128 + 16
        'pointnext'   the same with the row of cls2partembed (16 x 50) instead        64 + 128 + 50
        'pointnext1'  ReLU(convc(row of cls2partembed))                              64

    In every form they are constant along the points of a cloud.  The reference expands them to (B, E, N) and concatenates;
    here they stay (B, E) and the finest FeaturePropogation takes them as a per-cloud term of its first conv (`cloud`),
    falling back to the reference's composition where the block has not the form for it."""

    def __init__(self, encoder_channel_list: List[int], decoder_layers: int = 2, decoder_blocks: List[int] = [1, 1, 1, 1],
                 decoder_strides: List[int] = [4, 4, 4, 4], act_args: str = 'relu', cls_map='pointnet2', num_classes: int = 16,
                 cls2partembed=None, **kwargs):
        super().__init__()
        self.decoder_layers = decoder_layers
        self.in_channels = encoder_channel_list[-1]
        skip_channels = encoder_channel_list[:-1]
        fp_channels = encoder_channel_list[:-1]

        self.conv_args = kwargs.get('conv_args', None)
        radius_scaling = kwargs.get('radius_scaling', 2)
        nsample_scaling = kwargs.get('nsample_scaling', 1)
        block = kwargs.get('block', 'InvResMLP')
        if isinstance(block, str):
            block = _BLOCKS[block]
        self.blocks = decoder_blocks
        self.strides = decoder_strides
        self.norm_args = kwargs.get('norm_args', {'norm': 'bn'})
        self.act_args = kwargs.get('act_args', {'act': 'relu'})  # (act_args is a named parameter: always this default)
        self.expansion = kwargs.get('expansion', 4)
        radius = kwargs.get('radius', 0.1)
        nsample = kwargs.get('nsample', 16)
        self.radii = self._to_full_list(radius, radius_scaling)
        self.nsample = self._to_full_list(nsample, nsample_scaling)
        self.cls_map = cls_map
        self.num_classes = num_classes
        self.use_res = kwargs.get('use_res', True)
        group_args = kwargs.get('group_args', {'NAME': 'ballquery'})
        self.aggr_args = kwargs.get('aggr_args', {'feature_type': 'dp_fj', "reduction": 'max'})
        if self.cls_map == 'curvenet':
            self.global_conv2 = nn.Sequential(create_convblock1d(fp_channels[-1] * 2, 128, norm_args=None, act_args=act_args))
            self.global_conv1 = nn.Sequential(create_convblock1d(fp_channels[-2] * 2, 64, norm_args=None, act_args=act_args))
            skip_channels[0] += 64 + 128 + 16
        elif self.cls_map == 'pointnet2':
            self.convc = nn.Sequential(create_convblock1d(16, 64, norm_args=None, act_args=act_args))
            skip_channels[0] += 64
        elif self.cls_map == 'pointnext':
            self.global_conv2 = nn.Sequential(create_convblock1d(fp_channels[-1] * 2, 128, norm_args=None, act_args=act_args))
            self.global_conv1 = nn.Sequential(create_convblock1d(fp_channels[-2] * 2, 64, norm_args=None, act_args=act_args))
            skip_channels[0] += 64 + 128 + 50
            self.cls2partembed = cls2partembed
        elif self.cls_map == 'pointnext1':
            self.convc = nn.Sequential(create_convblock1d(50, 64, norm_args=None, act_args=act_args))
            skip_channels[0] += 64
            self.cls2partembed = cls2partembed

        n = len(fp_channels)
        stages = [None] * n
        for i in range(-1, -n - 1, -1):
            # like the reference, the caller's group_args object is written to (pointnext.py:581-582, 598-599)
            group_args.radius = self.radii[i]
            group_args.nsample = self.nsample[i]
            stages[i] = self._make_dec(skip_channels[i], fp_channels[i], group_args=group_args, block=block, blocks=self.blocks[i])
        self.decoder = nn.Sequential(*stages)
        self.out_channels = fp_channels[-n]

    def _make_dec(self, skip_channels, fp_channels, group_args=None, block=None, blocks=1):
        radii, nsample = group_args.radius, group_args.nsample
        mlp = [skip_channels + self.in_channels] + [fp_channels] * self.decoder_layers
        layers = [FeaturePropogation(mlp, act_args=self.act_args)]
        self.in_channels = fp_channels
        for i in range(1, blocks):
            group_args.radius, group_args.nsample = radii[i], nsample[i]
            layers.append(block(self.in_channels, aggr_args=self.aggr_args, norm_args=self.norm_args, act_args=self.act_args,
                                group_args=group_args, conv_args=self.conv_args, expansion=self.expansion, use_res=self.use_res))
        return nn.Sequential(*layers)

    # one value per block of every decoder stage (pointnext.py:608-626): the encoder's rule on self.blocks / self.strides
    _to_full_list = PointNextEncoder_AMContrast3D._to_full_list

    def _levels(self):
        """(stage index, fine cloud index, coarse cloud index) in the reference's forward order: levels -1 .. -(n-1), then
        stage 0 between the clouds p[1] and p[2] (pointnext.py:657-663)"""
        return [(i, i - 1, i) for i in range(-1, -len(self.decoder), -1)] + [(0, 1, 2)]

    @torch.no_grad()
    def plan_geometry(self, p):
        """Coordinate-only half: per stage index {'fp': 3-NN indices / weights, 'blocks': one self-query plan per block
        after the FP module, on the stage's fine cloud; blocks with one grouper setting share a search}"""
        plans = {}
        for stage, fine, coarse in self._levels():
            cache, blocks = {}, []
            for blk in list(self.decoder[stage])[1:]:
                key = plan_key(blk.convs.grouper)
                if key not in cache:
                    cache[key] = blk.plan(p[fine])
                blocks.append(cache[key])
            plans[stage] = {'fp': FeaturePropogation.plan(p[fine], p[coarse]), 'blocks': blocks}
        return plans

    def class_channels(self, f, cls_label):
        """e (B, E): the class-conditioned channels of the finest level, one row per cloud"""
        device = f[-1].device
        if self.cls_map in ('curvenet', 'pointnext'):
            emb1 = torch.max(run_convblocks(self.global_conv1, f[-2]), dim=-1)[0]
            emb2 = torch.max(run_convblocks(self.global_conv2, f[-1]), dim=-1)[0]
            if self.cls_map == 'curvenet':
                tail = shape_one_hot(cls_label, self.num_classes, device)
            else:
                self.cls2partembed = self.cls2partembed.to(device)
                tail = self.cls2partembed[cls_label.reshape(-1)]
            return torch.cat((emb1, emb2, tail), dim=1)
        if self.cls_map == 'pointnet2':
            rows = shape_one_hot(cls_label, self.num_classes, device)
        else:
            self.cls2partembed = self.cls2partembed.to(device)
            rows = self.cls2partembed[cls_label.reshape(-1)]
        return run_convblocks(self.convc, rows.unsqueeze(-1)).squeeze(-1)

    def forward(self, p, f, cls_label, geometry=None):
        if geometry is None:
            geometry = self.plan_geometry(p)
        e = self.class_channels(f, cls_label)  # (from the encoder's f[-2], f[-1]: before the loop overwrites them)
        for stage, fine, coarse in self._levels():
            g = geometry[stage]
            mods = list(self.decoder[stage])
            out = mods[0]([p[fine], f[fine]], [p[coarse], f[coarse]], geom=g['fp'], cloud=e if stage == 0 else None)
            pf = [p[fine], out]
            for blk, gb in zip(mods[1:], g['blocks']):
                pf = blk(pf, geom=gb)
            f[fine if stage != 0 else -len(self.decoder) - 1] = pf[1]
        return f[-len(self.decoder) - 1]
