"""Part segmentation without a GPU: the registry holds BasePartSeg, PointNextPartDecoder, PointNet2PartDecoder and MultiSegHead,
every fixture variant has the reference's state-dict keys and shapes (tests/golden/partseg_state_keys.json, recorded from its
own classes by tools/record_partseg_fixtures.py), the channel arithmetic is the reference's, the decoder writes into the
caller's group_args as the reference does, the config variants build, the train loop sends part models to the eager loop, and
the NumPy restatement of the per-cloud-term conv (tests/cloud_term_ref.py) is the composition the reference runs -- expand the
class channels along the points, concatenate, convolve -- with its gradients folded accordingly."""
import json
import os

import numpy as np
import pytest
import torch

import cloud_term_ref as R
from conftest import GOLDEN

# tag: (config variant, width, keyword arguments of configs.model_cfg_partseg)
VARIANTS = {"pointnet2": ("pointnext-s", 8, {"cls_map": "pointnet2"}), "curvenet": ("pointnext-s", 8, {"cls_map": "curvenet"}),
            "pointnext": ("pointnext-s", 8, {"cls_map": "pointnext"}), "pointnext1": ("pointnext-s", 8, {"cls_map": "pointnext1"}),
            "blocks": ("pointnext-s", 8, {"cls_map": "pointnet2", "decoder_blocks": [2, 2, 1, 1]}),
            "pn2": ("pointnet++", 4, {}),
            "multi": ("pointnext-s", 8, {"cls_map": "pointnet2", "head": "MultiSegHead"})}
SEG_VARIANTS = [t for t in VARIANTS if t != "multi"]
E_OF = {"pointnet2": 64, "curvenet": 208, "pointnext": 242, "pointnext1": 64, "blocks": 64, "pn2": 16}


@pytest.fixture(scope="module")
def fix():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    z = np.load(os.path.join(GOLDEN, "partseg.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "partseg_state_keys.json")) as fh:
        d["keys"] = json.load(fh)
    return d


def fixture_cfg(tag, nsample=16):
    from amcontrast3d_amd import configs
    from openpoints.utils import EasyConfig
    variant, width, kw = VARIANTS[tag]
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_partseg(variant, num_classes=50, dropout=0, radius=0.1, nsample=nsample, width=width, global_feat=None,
                                         **kw))
    return cfg


def recorded_state(tag, fix):
    return {k: torch.from_numpy(fix["sd::%s::%s" % (k, "x".join(str(d) for d in shape))]) for k, shape in fix["keys"][tag]}


def fixture_model(tag, fix=None, nsample=16):
    """the model of the fixture (50 part classes, no dropout, radius 0.1, nsample 16, narrow widths); with `fix` its recorded weights"""
    from openpoints.models import build_model_from_cfg
    model = build_model_from_cfg(fixture_cfg(tag, nsample))
    if fix is not None:
        model.load_state_dict(recorded_state(tag, fix), strict=True)
    return model


def class_conv(model):
    """the class-conditioned conv: the first conv of the finest feature-propagation module"""
    dec = model.decoder
    return (dec.FP_modules[0] if hasattr(dec, "FP_modules") else dec.decoder[0][0]).convs[0][0]


def test_every_class_is_registered(fix):
    from openpoints.models.build import MODELS
    for name in ("BasePartSeg", "PointNextPartDecoder", "PointNet2PartDecoder", "MultiSegHead", "PointNextEncoder", "SegHead"):
        assert name in MODELS, name
    from openpoints.models.backbone import PointNet2PartDecoder, PointNextPartDecoder  # noqa: F401
    from openpoints.models.segmentation.base_seg import BasePartSeg, BaseSeg, MultiSegHead  # noqa: F401
    assert issubclass(BasePartSeg, BaseSeg)


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_state_dict_is_the_references(fix, tag):
    model = fixture_model(tag)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == fix["keys"][tag]
    model.load_state_dict(recorded_state(tag, fix), strict=True)
    names = [k for k, _ in got]
    if tag == "multi":
        assert "head.multi_shape_heads.15.1.bias" in names and "head.multi_shape_heads.0.0.1.running_var" in names
        assert [model.head.multi_shape_heads[i][-1].out_channels for i in range(16)] == model.head.num_parts
    elif tag == "pn2":
        assert "decoder.FP_modules.0.convs.0.0.weight" in names
    else:
        assert "decoder.decoder.0.0.convs.0.0.weight" in names
        assert ("decoder.convc.0.0.bias" in names) == (tag in ("pointnet2", "pointnext1", "blocks"))
        assert ("decoder.global_conv1.0.0.bias" in names) == (tag in ("curvenet", "pointnext"))
    if tag == "blocks":
        assert "decoder.decoder.0.1.pwconv.1.0.weight" in names and "decoder.decoder.1.1.convs.convs.0.0.weight" in names
        assert not any(k.startswith("decoder.decoder.2.1.") for k in names)


@pytest.mark.parametrize("tag", SEG_VARIANTS)
def test_channel_arithmetic_is_the_references(fix, tag):
    model = fixture_model(tag)
    assert list(model.encoder.channel_list) == fix[f"{tag}_channel_list"].tolist()
    assert model.decoder.out_channels == int(fix[f"{tag}_out_channels"])
    conv = class_conv(model)
    skip = 7 if tag == "pn2" else model.encoder.channel_list[0]
    up = model.encoder.channel_list[1] if tag != "pn2" else model.decoder.FP_modules[1].convs[-1][0].out_channels
    assert conv.in_channels == E_OF[tag] + skip + up, "class channels first, then the skip features, then the interpolated ones"
    assert model.head.head[0][0].in_channels == model.decoder.out_channels


def test_decoder_writes_into_the_callers_group_args(fix):
    """pointnext.py:581-582, 598-599: radius / nsample of the LAST stage built (the finest) are left in the caller's object"""
    from openpoints.models.backbone import PointNextPartDecoder
    from openpoints.utils import EasyConfig
    args = EasyConfig()
    args.update({"group": {"NAME": "ballquery", "normalize_dp": True}})
    dec = PointNextPartDecoder([8, 16, 32, 64, 128], decoder_blocks=[2, 1, 1, 1], decoder_strides=[2, 2, 2, 2], radius=0.1,
                               radius_scaling=2.5, nsample=16, group_args=args.group, conv_args={"order": "conv-norm-act"})
    assert dec.radii == [[0.1, 0.25], [0.25], [0.625], [1.5625]] and dec.nsample == [[16, 16], [16], [16], [16]]
    assert args.group.radius == 0.25 and args.group.nsample == 16, "the second block of stage 0 was the last one built"
    assert dec.decoder[0][1].convs.grouper.radius == 0.25 and len(dec.decoder[0]) == 2 and len(dec.decoder[1]) == 1
    lists = [[0.1], [0.2], [0.3], [0.4]]
    dec = PointNextPartDecoder([8, 16, 32, 64, 128], decoder_blocks=[2, 1, 1, 1], radius=lists, group_args=args.group,
                               conv_args={"order": "conv-norm-act"})
    assert lists == [[0.1, 0.1], [0.2], [0.3], [0.4]], "_to_full_list pads the caller's lists in place"
    assert dec.out_channels == 8 and dec.in_channels == 8


@pytest.mark.parametrize("variant", ["pointnext-s", "pointnet++", "assanet"])
@pytest.mark.parametrize("head", ["SegHead", "MultiSegHead"])
def test_config_variants_build(fix, variant, head):
    from amcontrast3d_amd import configs
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_partseg(variant, head=head, width=8 if variant == "assanet" else None))
    model = build_model_from_cfg(cfg)
    assert type(model).__name__ == "BasePartSeg" and type(model.head).__name__ == head
    assert type(model.decoder).__name__ == ("PointNextPartDecoder" if variant == "pointnext-s" else "PointNet2PartDecoder")
    if variant == "pointnext-s":
        assert model.encoder.strides == [1, 2, 2, 2, 2] and model.encoder.sa_layers == 3 and model.decoder.cls_map == "curvenet"
        assert model.encoder.radii == [[0.1], [0.1], [0.25], [0.625], [1.5625]]
    if variant == "assanet":  # the decoder's copy of the channel arithmetic agrees with the encoder's
        assert model.decoder.FP_modules[0].convs[0][0].in_channels == 8 + 16 + model.decoder.FP_modules[1].convs[-1][0].out_channels
        assert model.decoder.FP_modules[-1].convs[0][0].in_channels == sum(model.encoder.channel_list[-2:])
    table = configs.cls2partembed()
    assert table.shape == (16, 50) and table.sum(1).tolist() == configs.SHAPENETPART_NUM_PARTS and (table.sum(0) == 1).all()


def test_decoderless_branch_and_cpu_refusal(fix):
    from amcontrast3d_amd import configs
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    model = fixture_model("pointnet2")
    with pytest.raises(RuntimeError, match="GPU only"):
        model({"pos": torch.rand(1, 64, 3), "x": torch.rand(1, 7, 64), "cls": torch.zeros(1, 1, dtype=torch.int64)})
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_partseg("pointnext-s", width=8))
    cfg.decoder_args = None
    cfg.cls_args = None
    bare = build_model_from_cfg(cfg)
    assert bare.decoder is None and bare.head is None

    class Enc(torch.nn.Module):
        def forward_seg_feat(self, data):
            return [data["pos"]], [data["x"], data["x"] * 2]
    bare.encoder = Enc()
    x = torch.rand(1, 7, 5)
    assert torch.equal(bare(torch.rand(1, 5, 3), x), x * 2), "without a decoder the last entry of the feature list is returned"


def test_part_models_train_in_the_eager_loop(fix):
    from amcontrast3d_amd import train
    for tag in ("pointnet2", "pn2", "multi"):
        assert not train.has_stage_list(fixture_model(tag)), tag


@pytest.mark.parametrize("B,E,C1,Cout,P", [(3, 16, 5, 7, 33), (2, 242, 8, 8, 17), (1, 1, 1, 1, 1)])
def test_restatement_is_the_expand_and_concatenate_composition(B, E, C1, Cout, P):
    """fp64 torch autograd on W . [e expanded along the points ; x] against the restatement with c = e W_cls^T: the output,
    dx, the [W_cls | W_skip] gradient (dW_cls = dc^T e) and de = dc W_cls"""
    rng = np.random.default_rng(B * 100 + E)
    e, x, w, dy = rng.standard_normal((B, E)), rng.standard_normal((B, C1, P)), rng.standard_normal((Cout, E + C1)), \
        rng.standard_normal((B, Cout, P))
    et, xt, wt = (torch.from_numpy(a).requires_grad_(True) for a in (e, x, w))
    cat = torch.cat((et.unsqueeze(-1).expand(-1, -1, P), xt), dim=1)
    y = torch.nn.functional.conv1d(cat, wt.unsqueeze(-1))
    y.backward(torch.from_numpy(dy))
    w_cls, w_skip = w[:, :E], w[:, E:]
    got = R.forward(x, w_skip, e @ w_cls.T)
    np.testing.assert_allclose(got, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    dc, dx, dw = R.backward(x, w_skip, dy)
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.concatenate([dc.T @ e, dw], axis=1), wt.grad.numpy(), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(dc @ w_cls, et.grad.numpy(), rtol=1e-11, atol=1e-11)
    assert (R.forward_magnitude(x, w_skip, e @ w_cls.T) >= np.abs(got) - 1e-12).all()


def test_route_predicate_on_the_host(fix):
    """cloud_term_route inspects modules, shapes and devices only: CPU tensors, a bias, a missing norm or activation all say
    'composition'"""
    from openpoints.models.layers import cloud_term_route, create_convblock1d
    blk = create_convblock1d(16 + 4 + 6, 8, norm_args={"norm": "bn1d"}, act_args={"act": "relu"})
    f1, f2, e = torch.rand(2, 4, 10), torch.rand(2, 6, 5), torch.rand(2, 16)
    assert cloud_term_route(blk, f1, f2, e) == "composition", "CPU tensors"
    assert cloud_term_route(create_convblock1d(26, 8, norm_args=None, act_args={"act": "relu"}), f1, f2, e) == "composition"
