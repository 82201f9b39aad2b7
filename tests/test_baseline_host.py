"""The plain PointNeXt baseline (cfgs/{s3dis,scannet}/pointnext-xl.yaml with examples/segmentation/main.py) on the host: the
registry builds BaseSeg / PointNextEncoder / PointNextDecoder and the CrossEntropy criterion, the state dict is the one
BaseSeg_AMContrast3D has for the same arguments (the reference's two families share keys; tests/golden/state_keys.json pins
the AA side), and the geometry entry points take contrast_head=None.  No forward pass: there is no CPU one."""
import copy
import inspect

import pytest
import torch

import amcontrast3d_amd

amcontrast3d_amd.activate()
from openpoints.loss import build_criterion_from_cfg  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402


def pointnext_xl(dataset, width=64, blocks=(1, 4, 7, 4, 4)):
    """the `model:` block of cfgs/s3dis/pointnext-xl.yaml / cfgs/scannet/pointnext-xl.yaml"""
    scannet = dataset == "scannet"
    cls_args = {"NAME": "SegHead", "num_classes": 20 if scannet else 13, "in_channels": None, "norm_args": {"norm": "bn"}}
    if scannet:
        cls_args["global_feat"] = "max"
    return {
        "NAME": "BaseSeg",
        "encoder_args": {
            "NAME": "PointNextEncoder", "blocks": list(blocks), "strides": [1, 4, 4, 4, 4], "sa_layers": 1, "sa_use_res": False,
            "width": width, "in_channels": 7 if scannet else 4, "expansion": 4, "radius": 0.05 if scannet else 0.1, "nsample": 32,
            "aggr_args": {"feature_type": "dp_fj", "reduction": "max"},
            "group_args": {"NAME": "ballquery", "normalize_dp": True},
            "conv_args": {"order": "conv-norm-act"}, "act_args": {"act": "relu"}, "norm_args": {"norm": "bn"},
        },
        "decoder_args": {"NAME": "PointNextDecoder"},
        "cls_args": cls_args,
    }


def as_amcontrast3d(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["NAME"] = "BaseSeg_AMContrast3D"
    cfg["encoder_args"]["NAME"] = "PointNextEncoder_AMContrast3D"
    cfg["decoder_args"]["NAME"] = "PointNextDecoder_AMContrast3D"
    return cfg


def build(cfg):
    c = EasyConfig()
    c.update(copy.deepcopy(cfg))
    return build_model_from_cfg(c)


@pytest.mark.parametrize("dataset", ["s3dis", "scannet"])
def test_baseline_builds_with_the_state_dict_of_the_amcontrast3d_model(dataset):
    for width, blocks in [(8, (1, 1, 1, 1, 1)), (64, (1, 4, 7, 4, 4))]:  # a quick one and the shipped one
        _model_case(dataset, width, blocks)
    _criterion_and_geometry()


def _model_case(dataset, width, blocks):
    from openpoints.models.backbone import PointNextDecoder, PointNextEncoder
    from openpoints.models.segmentation import BaseSeg
    cfg = pointnext_xl(dataset, width, blocks)
    model = build(cfg)
    assert type(model) is BaseSeg and type(model.encoder) is PointNextEncoder and type(model.decoder) is PointNextDecoder
    assert [n for n, _ in model.named_children()] == ["encoder", "decoder", "head"]
    ncls, cin = (20, 7) if dataset == "scannet" else (13, 4)
    assert model.encoder.encoder[0][0].convs[0][0].in_channels == cin
    assert model.head.head[-1][0].out_channels == ncls
    assert (model.head.global_feat == ["max"]) if dataset == "scannet" else (model.head.global_feat is None)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in build(as_amcontrast3d(cfg)).state_dict().items()}
    assert list(got) == list(want), "same keys in the same order"
    assert got == want
    # the reference's signatures (pointnext.py:443, 457, 494; base_seg.py:160): what main.py and its importers call
    assert list(inspect.signature(PointNextEncoder.forward).parameters) == ["self", "p0", "f0"]
    assert list(inspect.signature(PointNextEncoder.forward_seg_feat).parameters)[:3] == ["self", "p0", "f0"]
    assert list(inspect.signature(PointNextDecoder.forward).parameters)[:3] == ["self", "p", "f"]
    assert list(inspect.signature(BaseSeg.forward).parameters) == ["self", "data"]


def _criterion_and_geometry():
    c = EasyConfig()
    c.update({"NAME": "CrossEntropy", "label_smoothing": 0.2})
    crit = build_criterion_from_cfg(c)
    assert isinstance(crit, torch.nn.CrossEntropyLoss) and crit.label_smoothing == 0.2 and crit.weight is None
    assert crit.reduction == "mean" and crit.ignore_index == -100 and not hasattr(crit, "contrast_head")
    c.update({"weight": torch.tensor([1.0, 2.0, 0.5]), "ignore_index": 2})  # (main.py:224-230 writes the class weights in)
    crit = build_criterion_from_cfg(c)
    assert torch.equal(crit.weight, torch.tensor([1.0, 2.0, 0.5])) and crit.ignore_index == 2
    # on the CPU it is torch's forward
    x, y = torch.randn(2, 3, 5), torch.randint(0, 3, (2, 5))
    want = torch.nn.functional.cross_entropy(x, y, torch.tensor([1.0, 2.0, 0.5]), ignore_index=2, label_smoothing=0.2)
    assert torch.equal(crit(x, y), want)
    # CrossEntropyAce keeps building torch's own class and ignoring label_smoothing
    c = EasyConfig()
    c.update({"NAME": "CrossEntropyAce", "label_smoothing": 0.2})
    ace = build_criterion_from_cfg(c)
    assert type(ace.creterion) is torch.nn.CrossEntropyLoss and ace.creterion.label_smoothing == 0.0
    from amcontrast3d_amd import geometry, ops, pipeline
    for fn in (geometry.precompute, geometry.precompute_rest):
        assert "contrast_head" in inspect.signature(fn).parameters
    assert "head" in inspect.signature(pipeline.GraphPipeline.__init__).parameters
    assert "contrast_head" in inspect.signature(pipeline.GeometryPrefetcher.__init__).parameters
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cross_entropy_general(x, y, -100, 0.2, None)
