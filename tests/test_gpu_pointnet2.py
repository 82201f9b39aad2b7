"""PointNet++ (SSG, MSG) and ASSANet on the GPU against what the reference's own classes computed on the CPU
(tests/golden/pointnet2.npz, tools/record_pointnet2_fixtures.py): logits in eval and train mode, the loss and the recorded
gradients with the recorded weights; the route of every ConvPool / ASSA layer and its agreement with the plain composition;
deterministic mode; two iterations of train_one_epoch; the multi-scale concatenation.

Tolerances.  Logits in both modes and the loss keep the bound of tests/test_gpu_baseline.py: 1e-4 of max(1, |value|).  No
variant needs more there (measured on the MI355X: eval logits 3-6e-8, train logits 4-8e-5, the loss to six digits).
The recorded gradients do need more than that file's 1e-4 of a tensor's own range, in every variant: the reference's own fp32
step lies further than that from the same step in fp64 (model.double(), measured when the fixture was recorded and stored in
it as <variant>_fp64_dev; max-pool arg-max flips and BatchNorm's division by small batch deviations at these narrow widths
amplify single roundings), and so does this build's, measured on the MI355X against the recorded fp32 gradients:

    variant   reference fp32 against its fp64 twin   this build against the recorded gradients   allowed (4 x the first)
    ssg       5.2e-03 of a tensor's range            1.3e-03 .. 2.4e-03                          2.1e-02
    msg       3.3e-04                                3.4e-05 .. 2.3e-04                          1.3e-03
    assa      9.6e-03                                4.1e-03 .. 9.7e-03                          3.8e-02

(the last conv of the head, behind no BatchNorm, agrees to 3e-6 in all three).  A gradient is allowed 4 x the reference's own
measured deviation of its variant; nothing else is widened.

Reproducibility.  A forward that differs in its last bits flips arg-maxes, and the gradients then move by their own size.
With ConvPool's narrow 1x1 convs on the convolution library, whose choice of kernel is made per session, msg measured 3.8e-4
in four sessions and 2.6e-3 in a fifth (above its 1.3e-3).  ConvPool therefore keeps every conv on this library's own kernels
(run_convblocks(library=False)): the forward has one set of bits, and two processes repeat the figures above to three digits
(what is left is the order of the float atomics in backward).  ASSANet never took that library and repeats in both modes;
PointNet++ is judged in default mode only, because these narrow layers have no deterministic route (grouping_operation's and
grouped_conv's backward scatter with float atomics and raise in deterministic mode).
"""
import copy
import os

import numpy as np
import pytest
import torch

from test_pointnet2_host import VARIANTS, fixture_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from conftest import GOLDEN  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    import json
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    z = np.load(os.path.join(GOLDEN, "pointnet2.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "pointnet2_state_keys.json")) as fh:
        d["keys"] = json.load(fh)
    return d


def _data(fix):
    return {"pos": torch.from_numpy(fix["pos"]).to(DEV), "x": torch.from_numpy(fix["x"]).to(DEV)}


def _operators(model):
    enc = model.encoder
    ops_ = [enc.stem.SA_CONFIG_operator] if getattr(enc, "stem_aggr", False) else []
    return ops_ + [la.SA_CONFIG_operator for sa in enc.SA_modules for la in sa.local_aggregations]


def _train_step(fix, tag, model):
    """train-mode logits (asserted under the baseline bound), the loss (likewise) -> the parameter gradients"""
    model.train()
    logits = model(_data(fix))
    loss = logits.square().mean()
    loss.backward()
    want = fix[f"{tag}_logits_train"]
    tol = 1e-4 * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(logits.detach().cpu().numpy() - want).max())
    print(f"{tag}: train logits differ by {err:.2e} (allowed {tol:.2e})")
    assert err <= tol
    want_loss = float(fix[f"{tag}_loss"])
    print(f"{tag}: loss {float(loss.detach()):.6f} against {want_loss:.6f}")
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    return {k: p.grad for k, p in model.named_parameters()}


def _gradient_errors(fix, tag, grads):
    out = {}
    for k in fix[f"{tag}_grad_names"].tolist():
        want = fix[f"{tag}_grad::{k}"]
        scale = float(np.abs(want).max())
        assert scale > 0, k
        out[k] = float(np.abs(grads[k].cpu().numpy() - want).max()) / scale
    return out


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_recorded_step(fix, tag):
    from amcontrast3d_amd import ops
    model = fixture_model(tag, fix).to(DEV)
    dev_grad = float(fix[f"{tag}_fp64_dev"][2])
    model.eval()
    with torch.no_grad():
        got = model(_data(fix)).cpu().numpy()
    want = fix[f"{tag}_logits_eval"]
    tol = 1e-4 * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{tag}: eval logits differ by {err:.2e} (allowed {tol:.2e})")
    assert got.shape == want.shape and err <= tol
    assert dev_grad > 1e-4, "the reference's own fp32 gradients are further than the baseline bound from fp64"
    tol_grad = 4 * dev_grad
    modes = [False] + ([True] if tag == "assa" else [])  # (ConvPool's composition and first_conv routes scatter with float
    for det in modes:                                     # atomics in backward: no deterministic route, they raise there)
        model = fixture_model(tag, fix).to(DEV)
        with ops.deterministic_mode(det):
            errors = _gradient_errors(fix, tag, _train_step(fix, tag, model))
        for k, e in errors.items():
            print(f"{tag}, deterministic={det}: gradient of {k} differs by {e:.2e} of its range (allowed {tol_grad:.2e})")
        worst = max(errors, key=errors.get)
        assert errors[worst] <= tol_grad, worst


def _expected_route(op, cin, K):
    """the rule ConvPool follows for 'dp_fj' + max on fp32 GPU features"""
    from amcontrast3d_amd import ops
    if op.feature_type != "dp_fj" or op.reduction != "max":
        return "composition"
    cout, n = op.convs[0][0].out_channels, len(op.convs)
    if n == 1 and ops.local_aggregation_supported(cout, K):
        return "pooled"
    if n >= 2 and len(op.convs[0]) == 3 and ops.grouped_conv_bn_supported(cout, K):
        return "first_block"
    return "first_conv" if ops.grouped_conv_supported(cin, cout) else "composition"


def _log_routes(operators):
    """-> list that receives (operator, route name) for every ConvPool.route call forward makes"""
    taken = []
    for op in operators:
        if hasattr(op, "route"):
            inner = op.route
            op.route = lambda f, geom, inner=inner, op=op: taken.append((op, inner(f, geom))) or taken[-1][1]
    return taken


@pytest.mark.parametrize("tag", ["ssg", "msg"])
def test_convpool_routes_of_the_fixture_models(fix, tag):
    model = fixture_model(tag, fix).to(DEV).train()
    operators = _operators(model)
    taken = _log_routes(operators)
    model(_data(fix))
    assert [t[0] for t in taken] == operators
    got = [t[1] for t in taken]
    want = [_expected_route(op, op.convs[0][0].in_channels - 3, 16) for op in operators]
    print(tag, got)
    assert got == want
    assert set(got) == {"composition", "first_conv"}, "nsample 16: the narrow stages compose, the last stage fuses gather and first conv"


def _standalone(aggr, channels, nsample, use_res, seed=0, radius=0.15):
    from openpoints.models.layers import LocalAggregation
    from openpoints.utils import EasyConfig
    a = EasyConfig()
    a.update({"aggr": aggr, "group": {"NAME": "ballquery", "radius": radius, "nsample": nsample, "normalize_dp": True},
              "conv": {"order": "conv-norm-act"}, "norm": {"norm": "bn"}, "act": {"act": "relu"}})
    torch.manual_seed(seed)
    return LocalAggregation(list(channels), a.aggr, a.conv, a.norm, a.act, a.group, use_res).to(DEV).train()


def _clouds(n=600, m=150, c=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    sup = torch.rand(2, n, 3, generator=g)
    pick = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(2)])
    qry = torch.gather(sup, 1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    f = torch.randn(2, c, n, generator=g)
    return sup.to(DEV), qry.to(DEV), pick.to(DEV), f.to(DEV)


def _compose_convpool(op, qry, sup, f, pick):
    """the reference's composition with the module's own (torch) layers: group, concatenate, convs, pool, residual"""
    from openpoints.models.layers import get_aggregation_feautres
    dp, fj = op.grouper(qry, sup, f)
    fi = torch.gather(f, -1, pick.unsqueeze(1).expand(-1, f.shape[1], -1))
    out = op.reduction_layer(op.convs(get_aggregation_feautres(qry, dp, fi, fj, op.feature_type)))
    return op.act(out + op.skipconv(fi)) if op.use_res else out


def _compose_assa(op, qry, sup, f, pick):
    """local_aggregation.py:118-138 with the module's own (torch) layers: the (B,3C,M,K) tensor and its reduction"""
    f = op.convs[:op.num_preconv](f)
    dp, fj = op.grouper(qry, sup, f)
    B, C, M, K = fj.shape
    x = (fj.unsqueeze(1).expand(-1, 3, -1, -1, -1) * dp.unsqueeze(2)).reshape(B, -1, M, K)
    out = op.convs[op.num_preconv:](op.reduction_layer(x))
    if not op.use_res:
        return out
    return op.act(out + op.skip_layer(torch.gather(f, -1, pick.unsqueeze(1).expand(-1, C, -1))))


def _same_within(a, b, what, tol=1e-4):
    scale = float(b.abs().max())
    err = float((a - b).abs().max()) / scale
    print(f"{what}: {err:.2e} of the range")
    assert scale > 0 and err <= tol, what


CONVPOOL = {"NAME": "convpool", "feature_type": "dp_fj", "reduction": "max"}
LAYERS = [("pooled", CONVPOOL, [8, 32], 32, False), ("first_block", CONVPOOL, [8, 32, 32, 64], 32, False),
          ("first_block", CONVPOOL, [8, 32, 64], 32, True), ("first_conv", CONVPOOL, [8, 32, 32, 64], 16, False),
          ("composition", CONVPOOL, [8, 16, 16, 24], 16, True),
          ("composition", {"NAME": "convpool", "feature_type": "dp_fj", "reduction": "mean"}, [8, 32, 32], 32, False),
          ("composition", {"NAME": "convpool", "feature_type": "dp_df", "reduction": "max"}, [8, 32, 32], 32, False),
          ("assa", {"NAME": "ASSA", "feature_type": "assa", "reduction": "mean"}, [8, 24, 24, 24], 32, True),
          ("assa", {"NAME": "ASSA", "feature_type": "assa", "reduction": "max"}, [8, 24, 24, 48], 16, True),
          ("assa", {"NAME": "ASSA", "feature_type": "assa", "reduction": "sum"}, [8, 24, 24, 24], 16, False)]


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: f"{l[0]}-{l[1]['reduction']}-{len(l[2]) - 1}convs-k{l[3]}{'-res' if l[4] else ''}")
def test_layer_route_agrees_with_the_composition(layer):
    """every route of ConvPool and the kernel route of ASSA against the reference's composition run with the same module's
    torch layers, forward and the gradients of the features and of every parameter, within 1e-4 of a tensor's range (the
    bound tests/test_gpu_layers.py applies to the PointNeXt blocks)"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    route, aggr, channels, nsample, use_res = layer
    la = _standalone(aggr, channels, nsample, use_res)
    twin = copy.deepcopy(la)
    op = la.SA_CONFIG_operator
    sup, qry, pick, f = _clouds()
    fa, fb = f.clone().requires_grad_(True), f.clone().requires_grad_(True)
    if route != "assa":
        taken = _log_routes([op])
    got = la(qry, sup, fa, pick)
    if route != "assa":
        assert [t[1] for t in taken] == [route] == [_expected_route(op, 8, nsample)]
        extras = route in ("pooled", "first_block")  # moments / reverse lists are planned only for the routes that read them
        plan = op.plan(qry, sup)
        assert (plan.get("mom") is not None) == extras and (plan.get("csr") is not None) == (route == "first_block")
        before = copy.deepcopy(la.state_dict())
        assert op.route(fa.detach(), plan) == route, "asking for the route launches nothing and moves no statistics"
        assert all(torch.equal(v, before[k]) for k, v in la.state_dict().items())
    want = (_compose_assa if route == "assa" else _compose_convpool)(twin.SA_CONFIG_operator, qry, sup, fb, pick)
    _same_within(got, want, "output")
    r = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (got * r).sum().backward()
    (want * r).sum().backward()
    _same_within(fa.grad, fb.grad, "feature gradient")
    want_grads = {k: q.grad for k, q in twin.named_parameters()}
    for k, p in la.named_parameters():
        q = want_grads[k]
        scale = float(q.abs().max())
        gamma = want_grads.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if gamma is not None and gamma.dim() == 1:  # a BatchNorm's d(beta) is judged on d(gamma)'s scale (sums of the same
            scale = max(scale, float(gamma.abs().max()))  # terms; before another BatchNorm d(beta) cancels to ~0)
        err = float((p.grad - q).abs().max()) / scale
        print(f"{k}: {err:.2e} of the range")
        assert scale > 0 and err <= 1e-4, k
    for a, b in zip(la.buffers(), twin.buffers()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), "running statistics advance as torch's do"


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled-identity", "no-identity"])
def test_group_all_convpool(pooled):
    """nsample None -> GroupAll, which has no plan: with use_pooled_as_identity the identity is the max over the one group
    (dp comes from the grouper's return), without it the layer aggregates the whole cloud and adds no identity"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    la = _standalone(dict(CONVPOOL, use_pooled_as_identity=pooled), [8, 16, 24], None, True)
    twin = copy.deepcopy(la).SA_CONFIG_operator
    sup, qry, _, f = _clouds()
    assert la.plan(qry[:, :1], sup) is None
    got = la(qry[:, :1].contiguous(), sup, f)
    dp, fj = twin.grouper(qry[:, :1], sup, f)
    want = twin.convs(torch.cat([dp, fj], 1)).max(-1)[0]
    want = twin.act(want + (twin.skipconv(fj.max(-1)[0]) if pooled else 0))
    assert got.shape == want.shape == (2, 24, 1)
    _same_within(got, want, "output")


def test_deterministic_mode_repeats_the_bits(fix):
    from amcontrast3d_amd import ops
    runs = []
    for _ in range(2):
        model = fixture_model("assa", fix).to(DEV).train()
        with ops.deterministic_mode():
            logits = model(_data(fix))
            logits.square().mean().backward()
        runs.append([logits.detach()] + [p.grad for p in model.parameters()])
    assert all(g is not None for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_two_iterations_of_train_one_epoch(fix, tag, monkeypatch):
    from amcontrast3d_amd import train
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import ConfusionMatrix, EasyConfig
    B, N, classes = 2, 1024, 5
    train.release_pipelines()
    torch.manual_seed(1)
    model = fixture_model(tag).to(DEV)
    cc = EasyConfig()
    cc.update({"NAME": "CrossEntropy"})
    crit = build_criterion_from_cfg(cc).to(DEV)
    cfg = EasyConfig()
    cfg.update({"num_classes": classes, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
                "grad_norm_clip": 10, "sched_on_epoch": False, "criterion_args": {"NAME": "CrossEntropy"}})
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(4)
    loader = []
    for _ in range(2):
        pos = rng.uniform(0, 0.7, (B, N, 3)).astype(np.float32)
        loader.append({"pos": torch.from_numpy(pos), "x": torch.from_numpy(rng.uniform(0, 1, (B, N, 3)).astype(np.float32)),
                       "heights": torch.from_numpy(pos[:, :, 2:].copy()), "y": torch.from_numpy(rng.integers(0, classes, (B, N)))})
    counted = []
    metrics = ConfusionMatrix.all_metrics
    monkeypatch.setattr(ConfusionMatrix, "all_metrics", lambda self: counted.append(int(self.value.sum())) or metrics(self))

    class Sched:
        calls = 0

        def step(self, epoch):
            Sched.calls += 1
    before = [p.detach().clone() for p in model.parameters()]
    assert not train.has_stage_list(model)
    out = train.train_one_epoch(model, loader, crit, opt, Sched(), None, 1, cfg)
    torch.cuda.synchronize()
    assert not train._PIPELINES, "no captured pipeline for these models yet"
    assert np.isfinite(out[0]) and Sched.calls == 2
    assert counted == [2 * B * N]
    unmoved = [k for (k, p), q in zip(model.named_parameters(), before) if torch.equal(p.detach(), q)]
    assert not unmoved, unmoved


def test_msg_concatenates_its_scales_in_order(fix):
    model = fixture_model("msg", fix).to(DEV).train()
    data = _data(fix)
    sa = model.encoder.SA_modules[0]
    plan = sa.plan(data["pos"])
    assert len(plan["blocks"]) == 2 and plan["blocks"][0]["idx"].shape == (2, 256, 16)
    new_p, out = sa(data["pos"], data["x"], geom=plan)
    widths = [la.SA_CONFIG_operator.convs[-1][0].out_channels for la in sa.local_aggregations]
    assert out.shape == (2, sum(widths), 256) and torch.equal(new_p, plan["new_p"])
    at = 0
    for la, w, g in zip(sa.local_aggregations, widths, plan["blocks"]):
        alone = la(plan["new_p"], data["pos"], data["x"], query_idx=plan["fps_idx"], geom=g)
        assert torch.equal(out[:, at:at + w], alone)
        at += w
    assert float(plan["blocks"][1]["dp"].abs().max()) > float(plan["blocks"][0]["dp"].abs().max()), "radius r, then 2r"
    # the plan the encoder builds for a whole batch is the one its forward builds for itself
    whole = model.encoder.plan_geometry(data["pos"])
    with torch.no_grad():
        a = model(dict(data))
        b = model({**data, "_geometry": {"encoder": whole, "decoder": model.decoder.plan_geometry(
            [data["pos"]] + [g["new_p"] for g in whole["modules"]])}})
    assert torch.equal(a, b)
