"""PointNet++ / ASSANet without a GPU: the registry builds every variant, state-dict keys and shapes are the reference's
(tests/golden/pointnet2_state_keys.json, recorded from its own classes by tools/record_pointnet2_fixtures.py), the channel
arithmetic is the reference's, a CPU forward is refused, the NumPy restatement of the separable aggregation
(tests/assa_ref.py) reproduces what the reference's ASSA fed its post-convolutions, the fixture clouds cover truncated and
padded ball-query rows, and train_one_epoch's route predicate sends these models to the eager loop."""
import json
import os

import numpy as np
import pytest
import torch

import assa_ref as R
from conftest import GOLDEN

VARIANTS = {"ssg": ("pointnet++", 4), "msg": ("pointnet++msg", 4), "assa": ("assanet", 9)}  # tag: (config variant, width)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def fix():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    z = np.load(os.path.join(GOLDEN, "pointnet2.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "pointnet2_state_keys.json")) as fh:
        d["keys"] = json.load(fh)
    return d


def fixture_model(tag, fix=None):
    """the model of the fixture (5 classes, no dropout, radius 0.1, nsample 16, narrow widths); with `fix` its recorded weights"""
    from amcontrast3d_amd import configs
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    variant, width = VARIANTS[tag]
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_pointnet2(variant, num_classes=5, dropout=0, radius=0.1, nsample=16, width=width))
    model = build_model_from_cfg(cfg)
    if fix is not None:
        model.load_state_dict({k: torch.from_numpy(fix[f"{tag}_sd::{k}"]) for k, _ in fix["keys"][tag]}, strict=True)
    return model


@pytest.mark.parametrize("variant", ["pointnet++", "pointnet++msg", "assanet", "assanet-l"])
def test_every_variant_builds_from_its_config(fix, variant):
    from amcontrast3d_amd import configs
    from openpoints.models import build_model_from_cfg
    from openpoints.models.backbone.pointnetv2 import PointNet2Decoder, PointNet2Encoder
    from openpoints.models.layers import ASSA, CHANNEL_MAP, ConvPool, LocalAggregation  # noqa: F401  (exported beside the old names)
    from openpoints.utils import EasyConfig
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_pointnet2(variant, width=8 if variant == "assanet-l" else None))
    model = build_model_from_cfg(cfg)
    assert type(model).__name__ == "BaseSeg" and isinstance(model.encoder, PointNet2Encoder)
    assert isinstance(model.decoder, PointNet2Decoder)
    ops = [la.SA_CONFIG_operator for sa in model.encoder.SA_modules for la in sa.local_aggregations]
    assert all(isinstance(o, ASSA if variant.startswith("assanet") else ConvPool) for o in ops)
    scales = {"pointnet++": 1, "pointnet++msg": 2, "assanet": 2, "assanet-l": 3}[variant]
    assert [len(sa.local_aggregations) for sa in model.encoder.SA_modules] == [scales] * 4
    if variant.startswith("assanet"):
        assert isinstance(model.encoder.stem.SA_CONFIG_operator, ASSA) and model.encoder.SA_modules[0].query_as_support


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_state_dict_is_the_references(fix, tag):
    model = fixture_model(tag)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == fix["keys"][tag]
    model.load_state_dict({k: torch.from_numpy(fix[f"{tag}_sd::{k}"]) for k, _ in fix["keys"][tag]}, strict=True)
    names = [k for k, _ in got]
    assert any(".SA_CONFIG_operator.convs.0.0.weight" in k for k in names)
    assert any(".SA_CONFIG_operator.convs.0.1.running_mean" in k for k in names)
    if tag == "assa":
        assert any(k.endswith(".SA_CONFIG_operator.skip_layer.weight") for k in names)


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_channel_arithmetic_is_the_references(fix, tag):
    model = fixture_model(tag)
    assert list(model.encoder.channel_list) == fix[f"{tag}_channel_list"].tolist()
    assert model.encoder.out_channels == int(fix[f"{tag}_out_channels"])


def test_convpool_skipconv_key():
    """use_res on a ConvPool whose width changes: the skip conv is a conv block without norm, key skipconv.0.*"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers import LocalAggregation
    from openpoints.utils import EasyConfig
    a = EasyConfig()
    a.update({"aggr": {"NAME": "convpool", "feature_type": "dp_fj", "reduction": "max"},
              "group": {"NAME": "ballquery", "radius": 0.1, "nsample": 8}, "conv": {"order": "conv-norm-act"},
              "norm": {"norm": "bn"}, "act": {"act": "relu"}})
    channels = [4, 8, 16]
    la = LocalAggregation(channels, a.aggr, a.conv, a.norm, a.act, a.group, True)
    assert channels == [7, 8, 16], "the caller's list is edited in place"
    keys = list(la.state_dict())
    assert keys[:2] == ["SA_CONFIG_operator.skipconv.0.weight", "SA_CONFIG_operator.skipconv.0.bias"]
    assert len(la.SA_CONFIG_operator.convs[1]) == 2, "no activation on the last conv of a residual block"
    channels = [6, 12, 12, 12]
    la = LocalAggregation(channels, {"NAME": "ASSA", "feature_type": "assa"}, a.conv, a.norm, a.act, a.group, True)
    assert channels == [6, 12, 12, 12] and la.SA_CONFIG_operator.num_preconv == 2  # ceil(12 / 3) * 3 = 12 again
    assert la.SA_CONFIG_operator.convs[1][0].out_channels == 4 and la.SA_CONFIG_operator.convs[2][0].in_channels == 12
    assert isinstance(la.SA_CONFIG_operator.skip_layer, torch.nn.Conv1d) and la.SA_CONFIG_operator.skip_layer.in_channels == 4


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_cpu_forward_is_refused(fix, tag):
    model = fixture_model(tag)
    with pytest.raises(RuntimeError, match="GPU only"):
        model({"pos": torch.rand(1, 64, 3), "x": torch.rand(1, 4, 64)})


def test_separable_aggregation_refuses_cpu_tensors(fix):
    from amcontrast3d_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.separable_aggregation(torch.rand(1, 4, 8), torch.zeros(1, 3, 2, dtype=torch.int32), torch.rand(1, 3, 3, 2))


@pytest.mark.parametrize("reduction", ["mean", "sum", "max"])
def test_restatement_reproduces_the_references_aggregation(fix, reduction):
    """sum / mean: torch reduces the K products in an order of its own: K product roundings, K - 1 adds and one division stay
    under (K + 1) * U * sum_k |dp * f| per element.  max involves no sum: exact."""
    f, idx, dp, want = fix["one_f"], fix["one_idx"], fix["one_dp"], fix[f"one_{reduction}_agg"]
    K = idx.shape[-1]
    got, arg = R.forward(f, idx, dp, reduction)
    assert got.shape == want.shape and got.dtype == np.float32
    if reduction == "max":
        np.testing.assert_array_equal(got, want)
        padded = (idx[:, :, 1:] == idx[:, :, :1]).any(-1)
        assert padded.any() and arg.max() < K
        return
    bound = (K + 1) * U * R.magnitude(f, idx, dp)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{reduction}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert np.abs(want).max() > 1e-3


def test_restatement_backward_is_the_gradient_of_its_forward():
    """fp64 twin against autograd of the reference's expression (expand, multiply, reduce) on random ball-like rows"""
    rng = np.random.default_rng(2)
    B, C, N, M, K = 2, 5, 40, 17, 6
    f, dp, g = rng.standard_normal((B, C, N)), rng.standard_normal((B, 3, M, K)), rng.standard_normal((B, 3 * C, M))
    idx = R.ball_like_idx(rng, B, M, K, N)
    for reduction in ("mean", "sum", "max"):
        ft = torch.from_numpy(f).requires_grad_(True)
        fj = torch.gather(ft, 2, torch.from_numpy(idx).long().reshape(B, 1, -1).expand(-1, C, -1)).reshape(B, C, M, K)
        x = (fj.unsqueeze(1).expand(-1, 3, -1, -1, -1) * torch.from_numpy(dp).unsqueeze(2)).reshape(B, -1, M, K)
        out = {"mean": x.mean(-1), "sum": x.sum(-1), "max": x.max(-1)[0]}[reduction]
        got, arg = R.forward(f, idx, dp, reduction, np.float64)
        np.testing.assert_allclose(got, out.detach().numpy(), rtol=1e-12, atol=1e-12)
        if reduction == "max":
            continue  # (ties on the padded rows: autograd and "first maximum" may name different, equal-valued, elements)
        out.backward(torch.from_numpy(g))
        np.testing.assert_allclose(R.backward(g, idx, dp, arg, reduction, N, np.float64), ft.grad.numpy(), rtol=1e-11, atol=1e-12)
    # max: the stored k alone carries the gradient
    got, arg = R.forward(f, idx, dp, "max", np.float64)
    df = R.backward(g, idx, dp, arg, "max", N, np.float64)
    want = np.zeros((B, N, C))
    for b in range(B):
        for m in range(M):
            for d in range(3):
                for c in range(C):
                    k = arg[b, d * C + c, m]
                    want[b, idx[b, m, k], c] += dp[b, d, m, k] * g[b, d * C + c, m]
    np.testing.assert_allclose(df, want.transpose(0, 2, 1), rtol=1e-11, atol=1e-12)


def test_fixture_clouds_cover_truncated_and_padded_rows(fix):
    """every stage and scale: >= 90 % of the queries have >= 4 distinct neighbours; every stage: some row is padded; stages
    0-2: some row holds more points in its radius than nsample (truncated)"""
    nsample = int(fix["meta"][2])
    for s in range(4):
        stage_truncated = stage_padded = 0
        for j in range(2):
            idx, cnt = fix[f"cover_idx_{s}_{j}"].astype(np.int64), fix[f"cover_cnt_{s}_{j}"]
            assert idx.shape[-1] == nsample and cnt.shape == idx.shape[:2]
            distinct = np.array([[len(set(row)) for row in cloud] for cloud in idx])
            share = float((distinct >= 4).mean())
            truncated, padded = int((cnt > nsample).sum()), int((distinct < nsample).sum())
            print(f"stage {s} scale {j}: {share:.1%} of queries with >= 4 distinct neighbours, {truncated} truncated, {padded} padded, "
                  f"{int((cnt == 0).sum())} empty")
            assert share >= 0.9
            stage_truncated, stage_padded = stage_truncated + truncated, stage_padded + padded
            assert (np.minimum(cnt, nsample) == distinct)[cnt > 0].all(), "a row holds min(in-radius count, nsample) distinct points"
        assert stage_padded >= 1 and (s > 2 or stage_truncated >= 1), s


def test_route_predicate_of_the_train_loop(fix):
    from amcontrast3d_amd import configs, train
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    for tag in VARIANTS:
        assert not train.has_stage_list(fixture_model(tag)), tag
    cfg = EasyConfig()
    cfg.update(configs.model_cfg("S"))
    pointnext = build_model_from_cfg(cfg)
    assert train.has_stage_list(pointnext)
    assert train.has_stage_list(torch.nn.DataParallel(pointnext)) and not train.has_stage_list(torch.nn.DataParallel(fixture_model("ssg")))
