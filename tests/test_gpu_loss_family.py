"""The plain criteria of openpoints.loss on the GPU: the two point-loss kernel families (csrc/loss.hip, pl_softmax_* and
pl_sigmoid_*) through the registry's modules, against the fp64 restatement of tests/loss_family_ref.py, at the bounds of
cross_entropy_general (tests/test_gpu_baseline.py:66-67): value within 1e-5 max(1, |want|), gradient within
1e-6 max(1, 10 max|grad|).  Then the edge rows, what dropped points may not influence, repeatability, graph capture and
train.train_one_epoch with SmoothCrossEntropy and with MaskedCrossEntropy (a 'mask' key in the batches).

The train-loop checks compare the captured pipeline with the eager loop at lr = 0, like the first epoch of
tests/test_gpu_baseline.py: with lr > 0 two runs of one loop drift apart by more than any bound that still says something
(tests/test_gpu_train_edges.py has the figures), and what this file adds to the step is the criterion -- its value in the
returned average and its gradient in every parameter's -- which lr = 0 shows in full.
"""
import functools

import numpy as np
import pytest
import torch

import loss_family_ref as lf
from test_baseline_host import build, pointnext_xl
from test_gpu_train_edges import GRAD_BOUND, _Probe, _grad_error, _grads, _loader, _same_results, _same_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIGMOID = ("BCELogits", "Poly1FocalLoss")


def _build(name, **kwargs):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.utils import EasyConfig
    cfg = EasyConfig()
    cfg.update(dict(kwargs, NAME=name))
    return build_criterion_from_cfg(cfg).to(DEV)


def _run(form, logits, target, mask, scale=0.7):
    """the module on the device -> (loss, gradient of scale * loss) on the CPU; asserts that the form's kernels were the route"""
    from amcontrast3d_amd import timing
    crit = _build(form["cls"], **form["kwargs"])
    x = logits.to(DEV).requires_grad_(True)
    family = "sigmoid" if form["cls"] in SIGMOID else "softmax"
    with timing.count_calls() as calls:
        loss = crit(x, target.to(DEV), mask.to(DEV)) if form["cls"] == "MaskedCrossEntropy" else crit(x, target.to(DEV))
        (loss * scale).backward()
    assert calls[f"point_loss_{family}_forward"] == 1 and calls[f"point_loss_{family}_backward"] == 1, (form["id"], dict(calls))
    return loss.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def _want(form_id, C, N, scale=0.7):
    form = {f["id"]: f for f in lf.forms(C)}[form_id]
    logits, target, mask = lf.inputs(C, N, form["labels"])
    return lf.evaluate(form, logits, target, mask, scale=scale)


def _compare(case, got, got_grad, want, want_grad):
    """the bounds of the module docstring; a NaN (SmoothCrossEntropy's eps / (C - 1) at C = 1) has to be a NaN on both sides"""
    nan = torch.isnan(want_grad)
    assert bool(torch.isnan(got)) == bool(torch.isnan(want)) and torch.equal(torch.isnan(got_grad), nan), f"{case}: NaN pattern"
    if bool(torch.isnan(want)):
        print(f"{case}: NaN on both sides")
        return
    err = abs(float(got) - float(want))
    gmax = float(want_grad.abs().max())
    gerr = float((got_grad.double() - want_grad).abs().max())
    print(f"{case}: loss {float(want):.6f} off by {err:.2e}, gradient off by {gerr:.2e} (max {gmax:.2e})")
    assert err <= 1e-5 * max(1.0, abs(float(want))), case
    assert gerr <= 1e-6 * max(1.0, 10 * gmax), case


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
@pytest.mark.parametrize("C", [1, 2, 13, 50])
def test_value_and_gradient_match_the_restatement_in_float64(C, N):
    """every form of every class; 1000 points span four blocks per cloud, so the partial sums and the finalize launch carry the
    result.  The pow forms (FocalLoss gamma = 0.5, Poly1FocalLoss gamma = 1.5) are held to the same bounds as the others."""
    for form in lf.forms(C):
        logits, target, mask = lf.inputs(C, N, form["labels"])
        got, got_grad = _run(form, logits, target, mask)
        _compare(f"{form['id']} C={C} N={N}", got, got_grad, *_want(form["id"], C, N))


def _edge(form, logits, target, mask):
    got, got_grad = _run(form, logits, target, mask, scale=1.0)
    want, want_grad = lf.evaluate(form, logits, target, mask)
    return got, got_grad, want, want_grad


def test_edge_rows():
    C, N = 13, 300
    by_id = {f["id"]: f for f in lf.forms(C)}
    # nothing counted: 0 / 0 = NaN and a zero gradient, as torch's mean over no rows
    logits, target, mask = lf.inputs(C, N, "ignore3")
    for fid, tgt, msk in (("smooth_ignore3", torch.full_like(target, 3), mask), ("masked", torch.full_like(target, -100), mask),
                          ("masked", lf.inputs(C, N)[1], torch.zeros_like(mask))):
        got, got_grad, want, want_grad = _edge(by_id[fid], logits, tgt, msk)
        assert torch.isnan(got) and torch.isnan(want), fid
        assert float(got_grad.abs().sum()) == 0.0 and float(want_grad.abs().sum()) == 0.0, fid
    # exactly one counted point
    one = torch.full_like(target, 3)
    one[1, 77] = 5
    one_mask = torch.zeros_like(mask)
    one_mask[1, 77] = 1
    for fid, tgt, msk in (("smooth_ignore3", one, mask), ("masked", lf.inputs(C, N)[1], one_mask)):
        got, got_grad, want, want_grad = _edge(by_id[fid], logits, tgt, msk)
        _compare(f"{fid}, one counted point", got, got_grad, want, want_grad)
        rows = got_grad.transpose(1, 2).reshape(-1, C)
        assert int((rows.abs().sum(1) > 0).sum()) == 1 and float(rows[N + 77].abs().sum()) > 0, fid
    for form in lf.forms(C):
        # logits of +-80: nothing overflows, the sigmoid family stays finite
        logits, target, mask = lf.inputs(C, N, form["labels"])
        big = torch.where(logits > 0, 80.0, -80.0)
        got, got_grad, want, want_grad = _edge(form, big, target, mask)
        assert torch.isfinite(got) and bool(torch.isfinite(got_grad).all()), form["id"]
        _compare(f"{form['id']}, logits of +-80", got, got_grad, want, want_grad)
        # a label that lands on class C: left out, zero gradient row (raw label C + 1 where the form remaps)
        out = target.clone()
        out[0, 5] = C if form["labels"] == "plain" else C + 1
        out_mask = mask.clone()
        out_mask[0, 5] = 1
        got, got_grad, want, want_grad = _edge(form, logits, out, out_mask)
        _compare(f"{form['id']}, a label of C", got, got_grad, want, want_grad)
        assert float(got_grad[0, :, 5].abs().sum()) == 0.0 and float(want_grad[0, :, 5].abs().sum()) == 0.0, form["id"]


def test_dropped_points_do_not_matter():
    """other logits and labels at ignored / masked-out points: same bits in the loss and in every other gradient row"""
    C, N = 13, 1000
    by_id = {f["id"]: f for f in lf.forms(C)}
    for fid in ("smooth_ignore3", "masked"):
        logits, target, mask = lf.inputs(C, N, by_id[fid]["labels"])
        dropped = (target == 3) if fid == "smooth_ignore3" else (mask != 1)
        assert 0 < int(dropped.sum()) < dropped.numel()
        noise = torch.randn(logits.shape, generator=torch.Generator().manual_seed(3)) * 50
        logits2 = torch.where(dropped[:, None, :], noise, logits)
        target2 = target if fid == "smooth_ignore3" else torch.where(dropped, (target + 5) % (C + 4), target)
        mask2 = torch.where(dropped, torch.tensor(7), mask) if fid == "masked" else mask
        a, ga = _run(by_id[fid], logits, target, mask)
        b, gb = _run(by_id[fid], logits2, target2, mask2)
        kept = ~dropped[:, None, :].expand_as(ga)
        assert torch.equal(a, b) and torch.equal(ga[kept], gb[kept]) and float(gb[~kept].abs().sum()) == 0.0, fid


def test_same_bits_on_repeat_and_under_deterministic_mode():
    from amcontrast3d_amd import ops
    C, N = 13, 1000
    for form in lf.forms(C):
        logits, target, mask = lf.inputs(C, N, form["labels"])
        first = _run(form, logits, target, mask)
        again = _run(form, logits, target, mask)
        with ops.deterministic_mode():
            det = _run(form, logits, target, mask)
        for other in (again, det):
            assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1]), form["id"]


@pytest.mark.parametrize("form_id", ["smooth_weight", "poly1focal_default"])
def test_forward_and_backward_replay_from_a_graph(form_id):
    """one softmax-family and one sigmoid-family form, captured on a side stream; a replay on new inputs is the eager result"""
    C, N = 13, 1000
    form = {f["id"]: f for f in lf.forms(C)}[form_id]
    crit = _build(form["cls"], **form["kwargs"])
    batches = [lf.inputs(C, N, form["labels"], seed=s) for s in (0, 1)]
    assert not torch.equal(batches[0][0], batches[1][0])
    x = batches[0][0].to(DEV).requires_grad_(True)
    t = batches[0][1].to(DEV).clone()

    def step():
        loss = crit(x, t)
        return loss, torch.autograd.grad(loss, x)[0]
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        step()  # (the first call also moves the module's plain-tensor tables to the device: not a thing to capture)
    torch.cuda.current_stream(DEV).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (captures on a side stream of its own)
        loss, grad = step()
    for logits, target, _ in batches[::-1]:
        with torch.no_grad():
            x.copy_(logits.to(DEV))
            t.copy_(target.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        lg = logits.to(DEV).requires_grad_(True)
        want = crit(lg, target.to(DEV))
        want.backward()
        assert torch.isfinite(want) and torch.equal(loss, want.detach()) and torch.equal(grad, lg.grad)


def test_multi_shape_cross_entropy_runs_its_inner_criterion_on_the_kernels():
    from amcontrast3d_amd import timing
    g = torch.Generator().manual_seed(9)
    shapes = [torch.randn(3, 13, 200, generator=g) * 3, torch.randn(3, 4, 200, generator=g) * 3]
    shape_labels = torch.tensor([1, 0, 1])
    points = torch.stack([torch.randint(0, 4, (200,), generator=g), torch.randint(0, 13, (200,), generator=g),
                          torch.randint(0, 4, (200,), generator=g)])
    ref = [s.double().requires_grad_(True) for s in shapes]
    want = lf.multi_shape(lf.smooth_cross_entropy, ref, points, shape_labels)
    want.backward()
    xs = [s.to(DEV).requires_grad_(True) for s in shapes]
    crit = _build("MultiShapeCrossEntropy", criterion_args={"NAME": "SmoothCrossEntropy"})
    with timing.count_calls() as calls:
        got = crit(xs, points.to(DEV), shape_labels.to(DEV))
        got.backward()
    assert calls["point_loss_softmax_forward"] == 3 and calls["point_loss_softmax_backward"] == 3
    for i in range(2):
        _compare(f"multishape, shape {i}", got.detach().cpu(), xs[i].grad.cpu(), want.detach(), ref[i].grad)


# ---- training -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _fresh_pipelines():
    from amcontrast3d_amd import train
    train.release_pipelines()
    yield
    train.release_pipelines()


def _make(name, graph_pipeline):
    """the tiny baseline model (width 8), the criterion from the registry, the fields main.py's loop reads, FusedAdamW at lr = 0"""
    from openpoints.optim import build_optimizer_from_cfg
    from openpoints.utils import EasyConfig
    cfg = pointnext_xl("s3dis", width=8, blocks=(1, 1, 1, 1, 1))
    cfg["cls_args"]["dropout"] = 0
    torch.manual_seed(0)
    model = build(cfg).to(DEV)
    crit = _build(name)
    c = EasyConfig()
    c.update({"num_classes": 13, "ignore_index": None, "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1,
              "grad_norm_clip": 10, "sched_on_epoch": False, "fps_lanes": 2, "criterion_args": {"NAME": name},
              "graph_pipeline": graph_pipeline})
    opt = build_optimizer_from_cfg(model, NAME="adamw", lr=0.0, weight_decay=1e-4)
    return model, crit, c, opt


def _batches(first, masked):
    out = _loader([(2, 1024)] * 4, first=first)
    for k, d in enumerate(out):
        if masked:
            d["mask"] = (torch.rand(2, 1024, generator=torch.Generator().manual_seed(first + k)) >= 0.2).long()
    return out


@pytest.mark.parametrize("name", ["SmoothCrossEntropy", "MaskedCrossEntropy"])
def test_train_one_epoch_on_the_captured_pipeline_is_the_eager_loop(name, monkeypatch):
    from amcontrast3d_amd import timing, train
    monkeypatch.setenv("AMC3D_AUDIT_GRAPHS", "1")  # building the pipeline raises on a memset node in any of its graphs
    masked = name == "MaskedCrossEntropy"
    model, crit, cfg, opt = _make(name, True)
    model2, crit2, cfg2, opt2 = _make(name, False)
    losses = []
    for epoch, first in ((1, 80), (2, 300)):
        seen, seen2 = [], []
        got = train.train_one_epoch(model, _batches(first, masked), crit, opt, _Probe(lambda k: seen.append(_grads(model))), None, epoch, cfg)
        torch.cuda.synchronize()
        assert len(train._PIPELINES) == 1, "one captured pipeline, built in the first epoch and reused in the second"
        hook = opt2.register_step_pre_hook(lambda o, a, kw: seen2.append(_grads(model2)))
        with timing.count_calls() as calls:
            want = train.train_one_epoch(model2, _batches(first, masked), crit2, opt2, _Probe(), None, epoch, cfg2)
        hook.remove()
        torch.cuda.synchronize()
        assert len(train._PIPELINES) == 1, "graph_pipeline = False builds none"
        assert calls["point_loss_softmax_forward"] == 4 and calls["point_loss_softmax_backward"] == 4, dict(calls)
        assert calls["cross_entropy_general_forward"] == 0 and calls["cross_entropy_forward"] == 0
        _same_results(got, want)
        _same_state(model, model2)
        assert len(seen) == len(seen2) == 4
        for k in range(4):
            assert _grad_error(seen[k], seen2[k], f"{name}, epoch {epoch}, update {k + 1}") <= GRAD_BOUND
        losses.append(got[0])
    assert np.isfinite(losses).all() and losses[0] != losses[1], "the second epoch's batches are other data"
    pipe = next(iter(train._PIPELINES.values()))[0]
    assert ("mask" in pipe.keys) == masked and pipe.head is None and pipe.tail is not None
    assert pipe.graph_nodes and not any(c.get("memset") for counts in pipe.graph_nodes.values() for c in counts)
