"""The plain PointNeXt baseline on the GPU: the general cross-entropy kernel (label smoothing, class weights, ignore_index)
against torch in float64, under graph capture, BaseSeg against BaseSeg_AMContrast3D with the same weights, and
train.train_one_epoch / evaluate.validate_boundary_inner with a model that returns the logits alone.

The training checks are those of tests/test_gpu_train_edges.py for the AA loop, with its helpers and its bounds, IMPORTED from
that file (its loader, scheduler probe, comparison helpers and GRAD_BOUND / GRAD_DISTINCT: an edit there changes these tests too --
intended for the bounds, to be remembered for the helpers; they belong in a shared module once that file may be touched): the reference
is the trainer's loop written out by hand (examples/segmentation/main.py:338-390) with torch's F.cross_entropy on a second,
identically seeded model.  As there, the parameters after an epoch are compared exactly with lr = 0 (weights untouched,
BatchNorm statistics advanced over all batches) together with the gradient of every update; with lr > 0 the interpolation
backward's float atomics make two runs of the SAME loop drift apart (that file's docstring has the figures), so a second epoch
with lr > 0 states what is exact: every update moves the parameters, and the first one's gradient is the hand loop's.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_baseline_host import as_amcontrast3d, build, pointnext_xl
from test_gpu_train_edges import (GRAD_BOUND, GRAD_DISTINCT, _Probe, _grad_distance, _grad_error, _grads, _loader, _params,
                                  _same_results, _same_state, _set_lr)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _ce_inputs(C, N, ignored, B=2):
    g = torch.Generator().manual_seed(C * 1000 + N)
    logits = torch.randn(B, C, N, generator=g) * 3
    target = torch.randint(0, C, (B, N), generator=g)
    weight = torch.rand(C, generator=g) * 1.5 + 0.5
    if ignored:
        target[torch.rand(B, N, generator=g) < 0.25] = 255
        target[0, 0] = C - 1  # at least one valid target
    return logits, target, weight


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("C", [1, 13, 20, 70])
def test_general_cross_entropy_matches_torch_in_float64(C, N):
    """value and gradient against F.cross_entropy on float64 CPU copies, at the tolerances of
    test_gpu_loss.py::test_cross_entropy_matches_torch; two calls on the same input give the same bits.
    (All targets ignored is not a case: the kernel then returns 0/0 = NaN and a zero gradient, as torch does.)"""
    from amcontrast3d_amd import ops
    for ignored in (False, True):
        logits, target, weight = _ce_inputs(C, N, ignored)
        ignore_index = 255 if ignored else -100
        for eps in (0.0, 0.2):
            for w in (None, weight):
                ref = logits.double().requires_grad_(True)
                want = F.cross_entropy(ref, target, None if w is None else w.double(), ignore_index=ignore_index,
                                       reduction="mean", label_smoothing=eps)
                (want * 0.7).backward()
                want = want.detach()
                runs = []
                for _ in range(2):
                    lg = logits.to(DEV).requires_grad_(True)
                    got = ops.cross_entropy_general(lg, target.to(DEV), ignore_index, eps, None if w is None else w.to(DEV))
                    (got * 0.7).backward()
                    runs.append((got.detach().cpu(), lg.grad.cpu()))
                case = f"C={C} N={N} eps={eps} weight={w is not None} ignored={ignored}"
                err = abs(float(runs[0][0]) - float(want))
                gerr = float((runs[0][1].double() - ref.grad).abs().max())
                print(f"{case}: loss {float(want):.6f} off by {err:.2e}, gradient off by {gerr:.2e} (max {float(ref.grad.abs().max()):.2e})")
                assert err <= 1e-5 * max(1.0, abs(float(want))), case
                assert gerr <= 1e-6 * max(1.0, float(ref.grad.abs().max()) * 10), case
                if ignored:
                    assert float(runs[0][1].transpose(1, 2)[target == 255].abs().sum()) == 0.0, case
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{case}: two runs differ"


def test_general_cross_entropy_without_an_ignore_index_and_with_a_label_out_of_range():
    """ignore_index=None (the C-ABI's has_ignore = 0): no value is special, -100 included.  A target outside [0, C) that is
    not the ignore value is left out like an ignored one -- the plain kernel's rule; torch raises a device-side assert there,
    so the reference is torch on the same targets with those labels set to its ignore value."""
    from amcontrast3d_amd import ops
    C, N = 13, 300
    logits, target, weight = _ce_inputs(C, N, False)
    bad = target.clone()
    bad[0, 5], bad[1, 7], bad[1, 8] = C, -3, -100
    for ignore_index, tgt, ref_tgt in ((None, target, target), (None, bad, torch.where((bad < 0) | (bad >= C), -100, bad)),
                                       (4, bad, torch.where((bad < 0) | (bad >= C), 4, bad))):
        ref = logits.double().requires_grad_(True)
        want = F.cross_entropy(ref, ref_tgt, weight.double(), ignore_index=-100 if ignore_index is None else ignore_index,
                               label_smoothing=0.2)
        want.backward()
        lg = logits.to(DEV).requires_grad_(True)
        got = ops.cross_entropy_general(lg, tgt.to(DEV), ignore_index, 0.2, weight.to(DEV))
        got.backward()
        assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
        assert float((lg.grad.cpu().double() - ref.grad).abs().max()) <= 1e-6 * max(1.0, float(ref.grad.abs().max()) * 10)
        left_out = (ref_tgt == (-100 if ignore_index is None else ignore_index))
        assert float(lg.grad.cpu().transpose(1, 2)[left_out].abs().sum()) == 0.0


def test_general_cross_entropy_replays_from_a_graph():
    """forward + backward captured once (one stream, no branches); every replay is the eager result bit for bit"""
    from amcontrast3d_amd import ops
    C, N = 13, 1000
    inputs = [_ce_inputs(C, N, True), _ce_inputs(C + 0, N + 0, True)]
    inputs[1] = (inputs[1][0].flip(2) * 0.5, inputs[1][1].flip(1), inputs[1][2])
    weight = inputs[0][2].to(DEV)
    x = inputs[0][0].to(DEV).requires_grad_(True)
    t = inputs[0][1].to(DEV).clone()

    def step():
        loss = ops.cross_entropy_general(x, t, 255, 0.2, weight)
        return loss, torch.autograd.grad(loss, x)[0]
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream(DEV).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
    for logits, target, _ in inputs[::-1]:
        with torch.no_grad():
            x.copy_(logits.to(DEV))
            t.copy_(target.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        lg = logits.to(DEV).requires_grad_(True)
        want = ops.cross_entropy_general(lg, target.to(DEV), 255, 0.2, weight)
        want.backward()
        assert torch.isfinite(want) and torch.equal(loss, want.detach()) and torch.equal(grad, lg.grad)
    assert not torch.equal(inputs[0][0], inputs[1][0])


def test_the_criterion_takes_the_kernel_only_with_smoothing_or_weights(monkeypatch):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd import ops
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.utils import EasyConfig
    calls, orig = [], ops.cross_entropy_general
    monkeypatch.setattr(ops, "cross_entropy_general", lambda *a: calls.append(a[2:4]) or orig(*a))
    logits, target, weight = (v.to(DEV) for v in _ce_inputs(13, 300, False))

    def crit(**kw):
        c = EasyConfig()
        c.update(dict({"NAME": "CrossEntropy"}, **kw))
        return build_criterion_from_cfg(c).to(DEV)
    for kw in ({"label_smoothing": 0.2}, {"weight": weight}, {"label_smoothing": 0.2, "weight": weight, "ignore_index": 3}):
        n = len(calls)
        got = crit(**kw)(logits, target)
        want = F.cross_entropy(logits, target, kw.get("weight"), ignore_index=kw.get("ignore_index", -100),
                               label_smoothing=kw.get("label_smoothing", 0.0))
        assert len(calls) == n + 1 and abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    n = len(calls)
    assert torch.equal(crit()(logits, target), F.cross_entropy(logits, target))                       # neither: torch, as before
    rows = logits.transpose(1, 2).reshape(-1, 13)
    assert torch.equal(crit(label_smoothing=0.2)(rows, target.flatten()), F.cross_entropy(rows, target.flatten(), label_smoothing=0.2))
    assert torch.equal(crit(label_smoothing=0.2, reduction="sum")(logits, target),
                       F.cross_entropy(logits, target, label_smoothing=0.2, reduction="sum"))
    assert len(calls) == n


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _twins(dataset):
    """BaseSeg and BaseSeg_AMContrast3D at the shape of the model_w8_blocks_b2_n1024 fixture (width 8, blocks [1,2,2,1,1],
    2 x 1024 points), one state dict in both; dropout = 0"""
    cfg = pointnext_xl(dataset, width=8, blocks=(1, 2, 2, 1, 1))
    cfg["cls_args"]["dropout"] = 0
    torch.manual_seed(0)
    aa = build(as_amcontrast3d(cfg)).to(DEV)
    base = build(cfg).to(DEV)
    base.load_state_dict(aa.state_dict())
    return base, aa


def _batch(dataset, b=2, n=1024, first_id=40):
    from amcontrast3d_amd import synthetic
    nb = {k: torch.from_numpy(v).to(DEV) for k, v in synthetic.make_batch(b, n, first_id=first_id).items()}
    if dataset == "scannet":  # 7 input channels (cfgs/scannet/pointnext-xl.yaml): colours, three more, height
        extra = torch.randn(b, 3, n, generator=torch.Generator().manual_seed(first_id)).to(DEV)
        nb["x"] = torch.cat([nb["x"][:, :3], extra, nb["x"][:, 3:]], dim=1).contiguous()
    return nb


@pytest.mark.parametrize("dataset", ["s3dis", "scannet"])
def test_baseline_model_is_the_amcontrast3d_model_without_its_stage_list(dataset):
    base, aa = _twins(dataset)
    data = _batch(dataset)
    with torch.no_grad():
        base.eval(), aa.eval()
        out = base(dict(data))
        assert torch.is_tensor(out) and out.shape == (2, 20 if dataset == "scannet" else 13, 1024)
        assert torch.equal(out, aa(dict(data))[0]), "eval(): same kernels on the same inputs"
    base.train(), aa.train()
    logits, (logits_aa, _) = base(dict(data)), aa(dict(data))
    assert torch.equal(logits, logits_aa), "train(): same kernels on the same inputs"
    r = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    (logits * r).sum().backward()
    (logits_aa * r).sum().backward()
    # The two backward passes run the same kernels on the same tensors; the bound is test_gpu_layers.py's: 1e-4 of the tensor's
    # own range, a BatchNorm's d(beta) judged on d(gamma)'s scale (sums of the same terms; where another BatchNorm follows,
    # d(beta) cancels to ~0 analytically).  Bit equality was expected and does not hold on the MI355X (measured: differences of
    # 1e-6 of a tensor's range, in weights of every stage): no route differs between the two models -- the decoder's
    # interpolation backward (ops.three_interpolate's gradient) adds its rows with float atomics, whose order is not fixed from
    # one launch to the next, and everything upstream of it inherits the last bits.
    # One tensor is stated by name instead: the stem's conv bias.  The stem has no norm, so its conv keeps a bias, and every
    # consumer of the stem's output is a conv followed by a train-mode BatchNorm (SA1's grouped conv, the last decoder level's
    # first conv), which removes a per-channel constant: the true gradient is zero, and what comes out is the fp32 rounding of
    # a sum over the 2 x 1024 positions.  d(weight) of the same conv sums the same per-position terms times inputs of order 1,
    # so in BOTH models |d(bias)| has to stay below 1e-4 of d(weight)'s range; a relative comparison of two roundings of
    # zero says nothing.
    stem_bias, stem_weight = "encoder.encoder.0.0.convs.0.0.bias", "encoder.encoder.0.0.convs.0.0.weight"
    named, grads_aa = dict(base.named_parameters()), {k: q.grad for k, q in aa.named_parameters()}
    assert stem_bias in named and stem_weight in named
    worst, where = 0.0, ""
    for k, p in named.items():
        q = grads_aa[k]
        assert (p.grad is None) == (q is None), k
        if q is None:
            continue
        if k == stem_bias:
            for which, g, w in (("baseline", p.grad, named[stem_weight].grad), ("AMContrast3D", q, grads_aa[stem_weight])):
                zero = float(g.abs().max()) / float(w.abs().max())
                print(f"{dataset}: {which} stem bias gradient {zero:.2e} of the stem weight gradient's range")
                assert zero <= 1e-4, (which, k)
            continue
        scale = float(q.abs().max())
        if k.endswith(".bias") and k[:-5] + ".weight" in named and named[k[:-5] + ".weight"].dim() == 1:
            scale = max(scale, float(grads_aa[k[:-5] + ".weight"].abs().max()))
        assert scale > 0, k
        err = float((p.grad - q).abs().max()) / scale
        if err > worst:
            worst, where = err, k
    print(f"{dataset}: worst parameter-gradient difference {worst:.2e} of a tensor's range ({where})")
    assert worst <= 1e-4, where


def test_validation_accepts_the_baseline_model():
    """evaluate.validate_boundary_inner(..., miou_B_I=False) is main.py's validate: same matrix, hence same metrics, as with
    the AMContrast3D model carrying the same weights"""
    from amcontrast3d_amd import evaluate
    base, aa = _twins("s3dis")
    batches = [_batch("s3dis", first_id=60 + 2 * k) for k in range(3)]
    got = evaluate.validate_boundary_inner(base, [dict(b) for b in batches], 13, None, 24, miou_B_I=False)
    want = evaluate.validate_boundary_inner(aa, [dict(b) for b in batches], 13, None, 24, miou_B_I=False)
    assert len(got) == len(want) == 5 and got[:3] == want[:3] and 0.0 < got[2] <= 100.0
    np.testing.assert_array_equal(np.asarray(got[3]), np.asarray(want[3]))
    np.testing.assert_array_equal(np.asarray(got[4]), np.asarray(want[4]))


# ---- training -----------------------------------------------------------------------------------------------------------------
CLASS_WEIGHTS = [1.0, 0.8, 1.3, 2.0, 0.6, 1.1, 0.9, 1.7, 0.5, 1.2, 1.4, 0.7, 1.6]


def _make(lr):
    """the tiny baseline model, CrossEntropy(label_smoothing=0.2, weight=w), the fields main.py's loop reads, FusedAdamW"""
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    cfg = pointnext_xl("s3dis", width=8, blocks=(1, 1, 1, 1, 1))
    cfg["cls_args"]["dropout"] = 0
    torch.manual_seed(0)
    model = build(cfg).to(DEV)
    cc = EasyConfig()
    cc.update({"NAME": "CrossEntropy", "label_smoothing": 0.2, "weight": torch.tensor(CLASS_WEIGHTS)})
    crit = build_criterion_from_cfg(cc).to(DEV)
    c = EasyConfig()
    c.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
              "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "criterion_args": {"NAME": "CrossEntropy"}})
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=lr, weight_decay=1e-4)
    assert type(opt).__name__ == "FusedAdamW"
    return model, crit, c, opt


def _hand_loop(model, cfg, opt, loader, scheduler, epoch=1):
    """examples/segmentation/main.py:338-390 written out, with torch's cross entropy -> (its return value, per update: the
    gradients before the clipping)"""
    from amcontrast3d_amd import train
    from openpoints.utils import ConfusionMatrix
    cm = ConfusionMatrix(num_classes=cfg.num_classes, ignore_index=cfg.ignore_index)
    weight = torch.tensor(CLASS_WEIGHTS, device=DEV)
    model.train()
    losses, raw = [], []
    for data in loader:
        data = {k: v.to(DEV) for k, v in data.items()}
        target = data["y"].squeeze(-1) if data["y"].dim() == 3 else data["y"]
        data["x"] = train.get_features_by_keys(data, cfg.feature_keys)
        logits = model(data)
        loss = F.cross_entropy(logits, target, weight, label_smoothing=0.2)
        loss.backward()
        raw.append(_grads(model))
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.grad_norm_clip, norm_type=2)
        opt.step()
        opt.zero_grad()
        scheduler.step(epoch)
        cm.update(logits.argmax(dim=1), target)
        losses.append(float(loss))
    return (float(np.mean(losses)),) + tuple(cm.all_metrics()), raw


@pytest.fixture(autouse=True)
def _fresh_pipelines():
    from amcontrast3d_amd import train
    train.release_pipelines()
    yield
    train.release_pipelines()


def _train_case(route, shapes, monkeypatch):
    from amcontrast3d_amd import train
    if route == "eager":
        monkeypatch.setenv("AMC3D_EAGER_TRAIN", "1")
    else:
        monkeypatch.setenv("AMC3D_AUDIT_GRAPHS", "1")  # building the pipeline raises on a memset node in any of its graphs
    n_same = sum(s == shapes[0] for s in shapes)
    model, crit, cfg, opt = _make(0.0)
    model2, _, cfg2, opt2 = _make(0.0)
    replayed, stepped = [], []  # gradients after each replayed step (the static tensors) / before each eager optimizer step
    sched = _Probe(lambda k: replayed.append(_grads(model)))
    hook = None if route == "captured" and n_same == len(shapes) else opt.register_step_pre_hook(lambda o, a, kw: stepped.append(_grads(model)))
    got = train.train_one_epoch(model, _loader(shapes), crit, opt, sched, None, 1, cfg)
    if hook is not None:
        hook.remove()
    torch.cuda.synchronize()
    want, raw = _hand_loop(model2, cfg2, opt2, _loader(shapes), _Probe())
    assert sched.calls == len(shapes) and sched.epochs == [1] * len(shapes)
    if route == "eager":
        assert not train._PIPELINES
        seen = stepped
    else:
        assert len(train._PIPELINES) == 1
        pipe = next(iter(train._PIPELINES.values()))[0]
        assert pipe.head is None and pipe.update_in_feature_graph and pipe.tail is not None
        assert all("loss" not in r for r in pipe.rest), "no loss geometry is planned for the plain step"
        assert pipe.graph_nodes and not any(c.get("memset") for counts in pipe.graph_nodes.values() for c in counts)
        seen = replayed[:n_same] + stepped[-(len(shapes) - n_same):] if n_same < len(shapes) else replayed
    assert len(seen) == len(raw) == len(shapes)
    _same_results(got, want)
    _same_state(model, model2)  # lr = 0: weights untouched, running statistics advanced identically over all batches
    for k in range(len(shapes)):
        assert _grad_error(seen[k], raw[k], f"{route}, update {k + 1}") <= GRAD_BOUND
        if k:
            assert _grad_distance(raw[k - 1], raw[k]) > GRAD_DISTINCT, "consecutive batches have different gradients"
    # another epoch, now training
    _set_lr(opt, 1e-3), _set_lr(opt2, 1e-3)
    model2.load_state_dict(model.state_dict())
    states, firsts = [_params(model)], []
    first_hook = opt.register_step_pre_hook(lambda o, a, kw: firsts.append(_grads(model))) if route == "eager" else None

    def each(k):
        states.append(_params(model))
        if route == "captured" and k == 1:
            firsts.append(_grads(model))
    got2 = train.train_one_epoch(model, _loader(shapes[:n_same], first=300), crit, opt, _Probe(each), None, 2, cfg)
    if first_hook is not None:
        first_hook.remove()
    torch.cuda.synchronize()
    assert np.isfinite(got2[0]) and len(states) == n_same + 1
    for k in range(n_same):
        assert any(not torch.equal(a, b) for a, b in zip(states[k], states[k + 1])), f"epoch 2, update {k + 1} (lr 1e-3) moved no parameter"
    _, raw2 = _hand_loop(model2, cfg2, opt2, _loader(shapes[:1], first=300), _Probe(), epoch=2)
    assert _grad_error(firsts[0], raw2[0], f"{route}, epoch 2, first update") <= GRAD_BOUND


@pytest.mark.parametrize("route", ["captured", "eager"])
def test_train_one_epoch_runs_the_plain_step(route, monkeypatch):
    _train_case(route, [(2, 1024)] * 6, monkeypatch)


def test_train_one_epoch_plain_step_with_a_ragged_last_batch(monkeypatch):
    _train_case("captured", [(2, 1024)] * 5 + [(1, 1024)], monkeypatch)
