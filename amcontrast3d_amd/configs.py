"""Model / loss configurations of the AMContrast3D-AA path as plain dicts.

The reference ships only the XL model (cfgs/s3dis/AMContrast3D-AA.yaml:32-64, blocks
[1,4,7,4,4], width 64, sa_layers 1); PointNeXt-S / -B / -L named by BASELINE.json are
the standard PointNeXt variants under the same schema:
S = blocks [1,1,1,1,1], width 32, sa_layers 2, sa_use_res True; L = [1,3,5,3,3],
width 32.  ``ambiguity_args`` are the values of cfgs/{s3dis,scannet}/AMContrast3D-AA.yaml:6-30.
Feed the dicts to ``openpoints.utils.EasyConfig().update(...)``.
"""
import copy

_VARIANTS = {
    #        blocks            width sa_layers sa_use_res
    'S': ([1, 1, 1, 1, 1], 32, 2, True),
    'B': ([1, 2, 3, 2, 2], 32, 1, False),
    'L': ([1, 3, 5, 3, 3], 32, 1, False),
    'XL': ([1, 4, 7, 4, 4], 64, 1, False),
}


def model_cfg(variant='S', num_classes=13, in_channels=4, dropout=0.5, radius=0.1, nsample=32, width=None,
              blocks=None, global_feat=None):
    b, w, sa_layers, sa_use_res = _VARIANTS[variant]
    cls_args = {'NAME': 'SegHead', 'num_classes': num_classes, 'in_channels': None, 'norm_args': {'norm': 'bn'},
                'dropout': dropout}
    if global_feat is not None:
        cls_args['global_feat'] = global_feat
    return copy.deepcopy({
        'NAME': 'BaseSeg_AMContrast3D',
        'encoder_args': {
            'NAME': 'PointNextEncoder_AMContrast3D',
            'blocks': list(blocks if blocks is not None else b),
            'strides': [1, 4, 4, 4, 4],
            'sa_layers': sa_layers,
            'sa_use_res': sa_use_res,
            'width': width if width is not None else w,
            'in_channels': in_channels,
            'expansion': 4,
            'radius': radius,
            'nsample': nsample,
            'aggr_args': {'feature_type': 'dp_fj', 'reduction': 'max'},
            'group_args': {'NAME': 'ballquery', 'normalize_dp': True},
            'conv_args': {'order': 'conv-norm-act'},
            'act_args': {'act': 'relu'},
            'norm_args': {'norm': 'bn'},
        },
        'decoder_args': {'NAME': 'PointNextDecoder_AMContrast3D'},
        'cls_args': cls_args,
    })


def model_cfg_mm(variant='XL', num_classes=13, in_channels=4, dropout=0.5, width=None, blocks=None, ignore_index=None,
                 dataset='s3dis', **apm):
    """AMContrast3D++ (cfgs/{s3dis,scannet}/AMContrast3D-MM.yaml:33-88): the AA model plus the ambiguity
    prediction module and masked refinement.  `apm`: overrides of the APM_args block."""
    cfg = model_cfg(variant, num_classes=num_classes, in_channels=in_channels, dropout=dropout, width=width, blocks=blocks)
    w = cfg['encoder_args']['width']
    cfg['NAME'] = 'BaseSeg_M_AMContrast3D'
    cfg['encoder_args']['NAME'] = 'PointNextEncoder_M_AMContrast3D'
    cfg['decoder_args']['NAME'] = 'PointNextDecoder_M_AMContrast3D'
    cfg['cls_args']['ignore_index'] = ignore_index
    cfg['AEF_args'] = ambiguity_args_mm(dataset)
    apm_args = {'NAME': 'APM_pf_ConCate', 'feature_dim': [w, 2 * w, 4 * w, 8 * w], 'linear_mapping': False,
                'cross_attention': False, 'feat_concate': False, 'channel': [32, 16, 8, 4, 2], 'dropout': [0, 0, 0, 0, 0],
                'nsample_k': 12, 'threshold': 0.9, 'threshold_max': 1.0, 'gamma': 1, 'fusion': 'MIN', 'att_dim': 3}
    apm_args.update(apm)
    cfg['APM_args'] = apm_args
    return copy.deepcopy(cfg)


def ambiguity_args_mm(dataset='s3dis'):
    """ambiguity_args of the MM configs: the AA values plus the regression weight and the refinement's source"""
    args = ambiguity_args(dataset)
    args.update({'w3': 0.01, 'source': 'APM', 'source_mode': 'Train'})
    return args


def criterion_cfg_mm():
    return {'NAME': 'CrossEntropyAcePre'}


def ambiguity_args(dataset='s3dis'):
    args = {
        'action': False, 'vis': False, 'nsample': 24, 'ccbeta': 0.04, 'cctype': 'Method2',
        'temperature': 0.3, 'supervisedCL': 'Method1', 'db': '-m', 'margin': 'adaptive',
        'mu': -1, 'nu': 0.5, 'miou_B_I': False, 'w1': 0.1, 'w2': 0.9, 'stages': 'up', 'stages_num': 4,
    }
    if dataset == 'scannet':  # cfgs/scannet/AMContrast3D-AA.yaml
        args.update({'temperature': 0.5, 'nu': 0.6})
    return args


def criterion_cfg():
    # cfgs/s3dis/default.yaml:59-61 (label_smoothing is accepted and ignored by CrossEntropyAce)
    return {'NAME': 'CrossEntropyAce', 'label_smoothing': 0.2}


SHAPENETPART_NUM_PARTS = [4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3]  # parts per shape category, 50 in all
_PARTSEG = ('pointnext-s', 'pointnet++', 'assanet')


def cls2partembed(num_parts=SHAPENETPART_NUM_PARTS):
    """(shape categories, parts) fp32 tensor: row s marks the parts of category s, which are numbered consecutively over the
    categories (ShapeNetPart's layout) -- what `cls_map: pointnext / pointnext1` index with the shape label"""
    import torch
    table = torch.zeros(len(num_parts), sum(num_parts))
    at = 0
    for s, n in enumerate(num_parts):
        table[s, at:at + n] = 1
        at += n
    return table


def model_cfg_partseg(variant='pointnext-s', num_classes=50, in_channels=7, dropout=0.5, radius=0.1, nsample=32, width=None,
                      cls_map='curvenet', decoder_blocks=None, head='SegHead', global_feat='max,avg', part_table=None):
    """BasePartSeg: part segmentation with the shape category as a second input.  The reference ships no YAML for it; these
    follow upstream OpenPoints' cfgs/shapenetpart as far as they can be reconstructed:

      'pointnext-s'  PointNextEncoder at strides [1,2,2,2,2] (many small clouds), sa_layers 3, sa_use_res, radius_scaling 2.5,
                     width 32, seven input channels (position, normal, height) + PointNextPartDecoder with `cls_map`
                     ('curvenet' upstream; 'pointnet2', 'pointnext', 'pointnext1') and `decoder_blocks` (default [1,1,1,1])
      'pointnet++'   PointNet2Encoder (single-scale, as model_cfg_pointnet2) + PointNet2PartDecoder
      'assanet'      the ASSANet encoder with its widths written out as `mlps` + PointNet2PartDecoder.  (Written out because
                     that decoder repeats the encoder's channel arithmetic from the shared arguments, and for
                     double_last_channel False the reference's two copies scale the width at different places.)

    head: 'SegHead' (num_classes part logits; train with CrossEntropy) or 'MultiSegHead' (one head per shape category; train
    with MultiShapeCrossEntropy).  part_table: the (16, 50) tensor of cls2partembed() for the 'pointnext*' maps (default: that)."""
    if variant not in _PARTSEG:
        raise KeyError(f"{variant!r}: one of {_PARTSEG}")
    if head == 'MultiSegHead':
        cls_args = {'NAME': 'MultiSegHead', 'num_classes': num_classes, 'in_channels': None, 'norm_args': {'norm': 'bn'},
                    'dropout': dropout}
    else:
        cls_args = {'NAME': 'SegHead', 'num_classes': num_classes, 'in_channels': None, 'norm_args': {'norm': 'bn'},
                    'dropout': dropout}
        if global_feat is not None:
            cls_args['global_feat'] = global_feat
    if variant == 'pointnext-s':
        enc = {'NAME': 'PointNextEncoder', 'blocks': [1, 1, 1, 1, 1], 'strides': [1, 2, 2, 2, 2], 'sa_layers': 3,
               'sa_use_res': True, 'width': width if width is not None else 32, 'in_channels': in_channels, 'expansion': 4,
               'radius': radius, 'radius_scaling': 2.5, 'nsample': nsample,
               'aggr_args': {'feature_type': 'dp_fj', 'reduction': 'max'},
               'group_args': {'NAME': 'ballquery', 'normalize_dp': True}, 'conv_args': {'order': 'conv-norm-act'},
               'act_args': {'act': 'relu'}, 'norm_args': {'norm': 'bn'}}
        dec = {'NAME': 'PointNextPartDecoder', 'cls_map': cls_map}
        if decoder_blocks is not None:
            dec['decoder_blocks'] = list(decoder_blocks)
        if cls_map in ('pointnext', 'pointnext1'):
            dec['cls2partembed'] = part_table if part_table is not None else cls2partembed()
    else:
        base = model_cfg_pointnet2(variant, num_classes=num_classes, in_channels=in_channels, dropout=dropout, radius=radius,
                                   nsample=nsample, width=width)
        enc, dec = base['encoder_args'], base['decoder_args']
        dec['NAME'] = 'PointNet2PartDecoder'
        if variant == 'assanet':
            w = enc['width']
            enc['mlps'] = [[[w << i] * 3 for _ in range(b)] for i, b in enumerate(enc['blocks'])]
    return copy.deepcopy({'NAME': 'BasePartSeg', 'encoder_args': enc, 'decoder_args': dec, 'cls_args': cls_args})


_POINTNET2 = ('pointnet++', 'pointnet++msg', 'assanet', 'assanet-l')


def model_cfg_pointnet2(variant='pointnet++', num_classes=13, in_channels=4, dropout=0.5, radius=0.1, nsample=32, width=None,
                        blocks=None, normalize_dp=None):
    """BaseSeg + PointNet2Encoder / PointNet2Decoder + SegHead: the PointNet++ and ASSANet baselines of the PointNeXt
    paper's tables.  The reference ships no YAML for them; these follow the encoder's docstring (pointnetv2.py:150-176) and
    upstream OpenPoints' cfgs/s3dis/{pointnet++,assanet,assanet-l}.yaml as far as they can be reconstructed:

      'pointnet++'     single-scale grouping, three convs per stage, widths w,w,2w / 2w,2w,4w / ... (w = 32), max pooling
      'pointnet++msg'  two scales per stage (radii r and 2r; the second scale's middle width is 1.5 x)
      'assanet'        ASSA blocks [2,2,2,2] of width 64, stem conv + stem aggregation, query_as_support, residuals,
                       double_last_channel False, mean reduction, relative positions divided by the radius; a stage's
                       output concatenates its blocks, so the width doubles per stage (2.4 M parameters with the head)
      'assanet-l'      width 128, blocks [3,3,3,3], widths tripling per stage (115.6 M parameters, the paper's figure)

    `width`, `blocks`, `radius` (doubling per stage) and `nsample` override the variant's values."""
    if variant not in _POINTNET2:
        raise KeyError(f"{variant!r}: one of {_POINTNET2}")
    enc = {'NAME': 'PointNet2Encoder', 'in_channels': in_channels, 'strides': [4, 4, 4, 4], 'layers': 3, 'radius': radius,
           'num_samples': nsample, 'sampler': 'fps', 'conv_args': {'order': 'conv-norm-act'}, 'act_args': {'act': 'relu'},
           'norm_args': {'norm': 'bn'}}
    if variant.startswith('assanet'):
        large = variant.endswith('-l')
        w = width if width is not None else (128 if large else 64)
        enc.update({'width': w, 'mlps': None, 'blocks': list(blocks if blocks is not None else ([3] * 4 if large else [2] * 4)),
                    'width_scaling': 3 if large else 2, 'radius_scaling': 2, 'block_radius_scaling': 1, 'use_res': True,
                    'stem_conv': True, 'stem_aggr': True, 'query_as_support': True, 'double_last_channel': False,
                    'aggr_args': {'NAME': 'ASSA', 'feature_type': 'assa', 'reduction': 'mean'},
                    'group_args': {'NAME': 'ballquery', 'normalize_dp': True if normalize_dp is None else normalize_dp}})
        dec = {'NAME': 'PointNet2Decoder', 'fp_mlps': [[w, w], [w, w], [2 * w, 2 * w], [4 * w, 4 * w]]}
    else:
        w = width if width is not None else 32
        if variant == 'pointnet++':
            mlps = [[[w << i, w << i, w << (i + 1)]] for i in range(4)]
            enc.update({'radius': radius, 'num_samples': nsample})
        else:
            mlps = [[[w << i, w << i, w << (i + 1)], [w << i, (w << i) * 3 // 2, w << (i + 1)]] for i in range(4)]
            enc.update({'radius': [[radius * 2 ** i, radius * 2 ** (i + 1)] for i in range(4)],
                        'num_samples': [[nsample, nsample] for _ in range(4)]})
        enc.update({'width': None, 'mlps': mlps, 'use_res': False,
                    'aggr_args': {'NAME': 'convpool', 'feature_type': 'dp_fj', 'reduction': 'max'},
                    'group_args': {'NAME': 'ballquery', 'normalize_dp': False if normalize_dp is None else normalize_dp}})
        dec = {'NAME': 'PointNet2Decoder', 'fp_mlps': [[4 * w, 4 * w, 4 * w], [8 * w, 4 * w], [8 * w, 8 * w], [8 * w, 8 * w]]}
    return copy.deepcopy({
        'NAME': 'BaseSeg', 'encoder_args': enc, 'decoder_args': dec,
        'cls_args': {'NAME': 'SegHead', 'num_classes': num_classes, 'in_channels': None, 'norm_args': {'norm': 'bn'},
                     'dropout': dropout}})
