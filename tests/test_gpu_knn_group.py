"""KNNGroup on the device: its coordinates (amc3d_knn_group_dp) against the fp32 restatement of group.py:309-320 in
tests/knn_group_ref.py, grouped features and their gradient, the neighbourhood layers with the k-NN grouper against
oracle.model_ref (whose ball-query `query_and_group` is swapped for the k-NN one with monkeypatch), and a whole model
through the captured pipeline.

Unnormalised dp is a gather and one subtraction: equal to the bit.  normalize_dp divides by the cloud's largest
sqrt((x*x + y*y) + z*z): one rounding of the divisor (the root) and one of the quotient may differ, 2 ulp; the largest
difference is printed.  Measured on an MI355X: 0 ulp in five of the ten normalised cases, 2 ulp in the other five --
torch.sqrt on the CPU is not correctly rounded (the restatement's maximum of the 300 / 77 cloud without relative_xyz is
1 ulp below the fp64 root rounded once, which is what the kernel's sqrtf gives; divided by the kernel's maximum the
restatement agrees to the bit)."""
import numpy as np
import pytest
import torch

import knn_group_ref as R
from test_gpu_knn_batch import dev, on_gpu, oracle, pair  # noqa: F401  (dev: fixture)
from test_gpu_layers import DEV, _cloud, _easy, _randomise, _run

pytestmark = pytest.mark.gpu


def _grouper(k, rel, norm, **kw):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers import create_grouper
    return create_grouper({'NAME': 'knn', 'nsample': k, 'relative_xyz': bool(rel), 'normalize_dp': bool(norm), **kw})


def _clouds(case):
    if case == "far-last":  # the farthest neighbour of the cloud belongs to the last query row (last thread of the last workgroup)
        sup, qry = pair("uniform", 300, 77)
        qry = qry.clone()
        qry[:, -1] += 5.0
        return sup, qry
    kind, n, m = case
    return pair(kind, n, m)


@pytest.mark.parametrize("rel", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("case", [("uniform", 300, 77), "far-last", ("dup", 300, 77), ("room", 2049, None), ("dup", 2048, None)])
def test_dp_against_the_restatement(dev, case, rel, norm):
    sup, qry = _clouds(case)
    k = 16 if sup.shape[1] > 300 else 9
    gs = sup.to(dev)
    gq = gs if qry is sup else qry.to(dev)
    g = _grouper(k, rel, norm)
    idx = g.query(gq, gs)
    want_idx, _ = R.oracle_knn(k, qry, sup)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx.numpy())
    dp, none = g(gq, gs)
    assert none is None and dp.shape == (2, 3, qry.shape[1], k) and dp.dtype == torch.float32
    want, _ = R.knn_group_forward(want_idx, qry, sup, None, bool(rel), bool(norm))
    if case == "far-last" and rel:
        norms = want.pow(2).sum(1).flatten(1)
        assert bool((norms.argmax(1) // k == qry.shape[1] - 1).all())
    ulp = R.ulp_diff(dp.cpu().numpy(), want.numpy())
    print(f"largest dp difference: {ulp} ulp")
    assert ulp <= (2 if norm else 0)
    assert torch.equal(g.relative_positions(idx, gq, gs), dp)
    assert torch.equal(_grouper(k, rel, norm, return_only_idx=True)(gq, gs), idx)


@pytest.mark.parametrize("det", [False, True])
def test_grouped_features_and_backward(dev, det):
    from amcontrast3d_amd import ops
    sup, qry = pair("uniform", 300, 77)
    gs, gq = sup.to(dev), qry.to(dev)
    feat = torch.randn(2, 5, 300, generator=torch.Generator().manual_seed(3))
    go = torch.randn(2, 5, 77, 9, generator=torch.Generator().manual_seed(4))
    want_idx, _ = oracle("uniform", 300, 77, 9)
    cf = feat.clone().requires_grad_(True)
    want_dp, want_fj = R.knn_group_forward(want_idx, qry, sup, cf, True, True)
    want_fj.backward(go)
    gf = feat.to(dev).requires_grad_(True)
    with ops.deterministic_mode(det):
        dp, fj = _grouper(9, 1, 1)(gq, gs, gf)
    assert not dp.requires_grad and torch.equal(fj.detach().cpu(), want_fj.detach())
    assert R.ulp_diff(dp.cpu().numpy(), want_dp.numpy()) <= 2
    if det:  # grouping_operation's scatter adds floats with atomics: the fused layers are the deterministic route
        with pytest.raises(RuntimeError, match="no deterministic route"):
            fj.backward(go.to(dev))
        return
    fj.backward(go.to(dev))
    np.testing.assert_allclose(gf.grad.cpu().numpy(), cf.grad.numpy(), rtol=0, atol=1e-5 * float(cf.grad.abs().max()))


# ------------------------------------------------------------------------------------------------------ layers
@pytest.fixture
def knn_oracle(monkeypatch):
    from oracle import model_ref
    monkeypatch.setattr(model_ref, "query_and_group", R.query_and_group)
    return model_ref


@pytest.mark.parametrize("nsample", [16, 32])
def test_set_abstraction_single_layer(knn_oracle, nsample):
    from openpoints.models.backbone.pointnext_blocks import SetAbstraction
    torch.manual_seed(1)
    p = _cloud(2, 4096, 0, 0.04)
    f = torch.randn(2, 32, p.shape[1], generator=torch.Generator().manual_seed(2))
    mod = SetAbstraction(32, 64, 1, 4, group_args=_easy(NAME='knn', nsample=nsample, normalize_dp=True),
                         norm_args={'norm': 'bn'}, act_args={'act': 'relu'}, conv_args={'order': 'conv-norm-act'},
                         feature_type='dp_fj', use_res=False).to(DEV).train()
    _randomise(mod, 3)
    pg = p.to(DEV)
    _run("blk", mod, lambda m, f: m([pg, f])[1],
         lambda sd, pool, f: knn_oracle.set_abstraction(sd, "blk", p, f, 4, None, nsample, 1, False, True, True, pool)[1],
         {"f": f}, 1, {"local_aggregation_forward": 1, "local_aggregation_backward": 1})


def test_inv_res_mlp(knn_oracle):
    from openpoints.models.backbone.pointnext_blocks import InvResMLP
    torch.manual_seed(4)
    p = _cloud(2, 4096, 1, 0.04)
    f = torch.randn(2, 64, p.shape[1], generator=torch.Generator().manual_seed(5))
    mod = InvResMLP(64, norm_args={'norm': 'bn'}, act_args={'act': 'relu'}, aggr_args={'feature_type': 'dp_fj', 'reduction': 'max'},
                    group_args=_easy(NAME='knn', nsample=32, normalize_dp=True),
                    conv_args={'order': 'conv-norm-act'}, expansion=4, use_res=True).to(DEV).train()
    _randomise(mod, 6)
    pg = p.to(DEV)
    _run("blk", mod, lambda m, f: m([pg, f])[1],
         lambda sd, pool, f: knn_oracle.inv_res_mlp(sd, "blk", p, f, None, 32, True, True, pool),
         {"f": f}, 1, {"local_aggregation_forward": 1, "local_aggregation_backward": 1, "bn_residual_forward": 1})


@pytest.mark.parametrize("nsample,calls", [(32, {"grouped_conv_bn_forward": 1, "sa_residual_forward": 1}), (24, {})])
def test_set_abstraction_two_layers_with_skip(knn_oracle, nsample, calls):
    """nsample 32: the fused first block; 24: the generic route"""
    from openpoints.models.backbone.pointnext_blocks import SetAbstraction
    torch.manual_seed(7)
    p = _cloud(2, 4096, 0, 0.04)
    f = torch.randn(2, 32, p.shape[1], generator=torch.Generator().manual_seed(8))
    mod = SetAbstraction(32, 64, 2, 4, group_args=_easy(NAME='knn', nsample=nsample, normalize_dp=True),
                         norm_args={'norm': 'bn'}, act_args={'act': 'relu'}, conv_args={'order': 'conv-norm-act'},
                         feature_type='dp_fj', use_res=True).to(DEV).train()
    _randomise(mod, 9)
    pg = p.to(DEV)
    _run("blk", mod, lambda m, f: m([pg, f])[1],
         lambda sd, pool, f: knn_oracle.set_abstraction(sd, "blk", p, f, 4, None, nsample, 2, True, True, True, pool)[1],
         {"f": f}, 1, calls)


# ------------------------------------------------------------------------------------------------------ whole model
def test_whole_model_through_the_captured_pipeline(monkeypatch):
    """the width-16 model of test_gpu_graph_pipeline._setup with group_args.NAME: knn -- two batches through GraphPipeline
    and through the eager step, that file's comparison: logits equal, loss within 1e-6"""
    import test_gpu_graph_pipeline as G
    from amcontrast3d_amd import configs
    plain = configs.model_cfg

    def knn_cfg(*a, **kw):
        cfg = plain(*a, **kw)
        cfg['encoder_args']['group_args']['NAME'] = 'knn'
        return cfg

    monkeypatch.setattr(configs, "model_cfg", knn_cfg)
    from openpoints.models.layers.group import KNNGroup, QueryAndGroup
    model, crit, aa, opt = G._setup(0.0, fused=False)
    groupers = [m for m in model.modules() if isinstance(m, (KNNGroup, QueryAndGroup))]
    assert len(groupers) >= 4 and all(isinstance(m, KNNGroup) for m in groupers)  # one per strided stage of PointNeXt-S
    src = G._batches(2)
    pipe, main = G._pipeline(model, crit, aa, opt, src[0], 2)
    got = []
    with torch.cuda.stream(main):
        for out in pipe.run(iter(src)):
            got.append((out["data"]["pos"].clone(), out["logits"].clone(), float(out["loss"])))
    torch.cuda.synchronize()
    assert len(got) == 2
    model2, crit2, aa2, opt2 = G._setup(0.0, fused=False)
    for i, (pos, logits, loss) in enumerate(got):
        assert torch.equal(pos, src[i]["pos"]), f"result {i} is not batch {i}"
        want_logits, want_loss = G._eager_step(model2, crit2, aa2, opt2, src[i])
        assert torch.equal(logits, want_logits), f"batch {i}: max {float((logits - want_logits).abs().max()):.2e}"
        assert abs(loss - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (i, loss, float(want_loss))
