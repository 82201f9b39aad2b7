"""The plain criteria of openpoints.loss on the CPU: the registry, the reference's signatures, and the numbers the reference's
own classes gave (tests/golden/loss_family.npz, recorded by tools/record_loss_fixtures.py) against the fp64 restatement
(tests/loss_family_ref.py) and against the product modules' torch-composition route.

Bounds.  The recorded numbers are fp32 evaluations: per point a log-softmax over at most 20 logits of magnitude <= ~12 and a
handful of products, each good to a few ulp (6e-8 relative), then an fp32 sum over 514 points whose error stays below
514 ulp / 2 of the result in the worst case and near sqrt(514) ulp in practice.  The project's bounds for cross_entropy_general
(value 1e-5 max(1, |want|), gradient 1e-6 max(1, 10 max|grad|)) lie an order of magnitude above that and are used here too.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import loss_family_ref as lf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("SmoothCrossEntropy", "MaskedCrossEntropy", "BCELogits", "FocalLoss", "Poly1CrossEntropyLoss", "Poly1FocalLoss",
         "MultiShapeCrossEntropy", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy")
B, N = 2, 257


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "loss_family.npz")))


def _build(name, **kwargs):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.utils import EasyConfig
    cfg = EasyConfig()
    cfg.update(dict(kwargs, NAME=name))
    return build_criterion_from_cfg(cfg)


def _recorded_cases(golden):
    """(form, C, logits, target, mask, loss, grad) for every recorded form"""
    for C in (13, 20):
        for form in lf.forms(C):
            key = f"{form['id']}/C{C}"
            if key + "/loss" not in golden:
                assert C == 20, key
                continue
            logits, target, mask = lf.inputs(C, N, form["labels"], B)
            pre = f"inputs/{form['labels']}/C{C}/"
            # the recorded inputs are the generator's: a drift of lf.inputs would otherwise compare two different problems
            assert np.array_equal(golden[pre + "logits"], logits.numpy()) and np.array_equal(golden[pre + "target"], target.numpy())
            assert np.array_equal(golden[pre + "mask"], mask.numpy())
            yield form, C, logits, target, mask, float(golden[key + "/loss"]), torch.from_numpy(golden[key + "/grad"]).double()


def _close(case, loss, grad, want, want_grad):
    err = abs(float(loss) - want)
    gerr = float((grad.double() - want_grad).abs().max())
    print(f"{case}: loss {want:.6f} off by {err:.2e}, gradient off by {gerr:.2e} (max {float(want_grad.abs().max()):.2e})")
    assert err <= 1e-5 * max(1.0, abs(want)), case
    assert gerr <= 1e-6 * max(1.0, 10 * float(want_grad.abs().max())), case


def test_every_name_is_registered_builds_and_has_the_reference_signature():
    """fails before the criteria exist: build_criterion_from_cfg({'NAME': 'SmoothCrossEntropy'}) raised KeyError"""
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    import openpoints.loss
    from openpoints.loss import LOSS
    with open(os.path.join(GOLDEN, "loss_family_signatures.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(NAMES)
    for name in NAMES:
        assert name in LOSS.module_dict, name
        kwargs = {"criterion_args": {"NAME": "SmoothCrossEntropy"}} if name == "MultiShapeCrossEntropy" else {}
        crit = _build(name, **kwargs)
        assert isinstance(crit, torch.nn.Module) and type(crit).__name__ == name
        for which, fn in (("init", type(crit).__init__), ("forward", type(crit).forward)):
            got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), p.kind.name]
                   for p in inspect.signature(fn).parameters.values() if p.name != "self"]
            assert got == recorded[name][which], (name, which, got)
    assert openpoints.loss.LabelSmoothingCrossEntropy is LOSS.module_dict["LabelSmoothingCrossEntropy"]
    assert openpoints.loss.SoftTargetCrossEntropy is LOSS.module_dict["SoftTargetCrossEntropy"]
    assert "DistillLoss" not in LOSS.module_dict
    # the attribute names the reference's classes expose
    smooth = _build("SmoothCrossEntropy", ignore_index=-100, num_classes=13, weight=lf.class_weights(13)[None])
    assert smooth.reducing_list.tolist() == [0] + list(range(14)), "negative ignore_index: every label >= 1 moves down by one"
    assert smooth.weight.dtype == torch.float32 and smooth.weight.shape == (13,) and not smooth.return_valid
    assert _build("SmoothCrossEntropy", ignore_index=3, num_classes=5).reducing_list.tolist() == [0, 1, 2, 0, 3, 4, 5]
    assert not hasattr(_build("SmoothCrossEntropy"), "reducing_list")
    assert isinstance(_build("MaskedCrossEntropy").creterion, torch.nn.CrossEntropyLoss)
    assert isinstance(_build("BCELogits", reduction="sum").criterion, torch.nn.BCEWithLogitsLoss)
    assert _build("FocalLoss", alpha=0.25).alpha.tolist() == [0.25, 0.75] and _build("FocalLoss").size_average is True
    assert isinstance(_build("MultiShapeCrossEntropy", criterion_args={"NAME": "CrossEntropy"}).criterion, torch.nn.CrossEntropyLoss)


def test_restatement_reproduces_the_reference(golden):
    n = 0
    for form, C, logits, target, mask, want, want_grad in _recorded_cases(golden):
        loss, grad = lf.evaluate(form, logits, target, mask)
        _close(f"{form['id']} C={C}", loss, grad, want, want_grad)
        n += 1
    assert n == 18 + 8


def test_product_modules_on_cpu_tensors_reproduce_the_reference(golden):
    """the torch-composition route; pins the label remap under a negative ignore_index, the eps / (C - 1) rule, the detached pt
    and Poly1's plain mean with class weights"""
    for form, C, logits, target, mask, want, want_grad in _recorded_cases(golden):
        crit = _build(form["cls"], **form["kwargs"])
        x = logits.clone().requires_grad_(True)
        loss = crit(x, target, mask) if form["cls"] == "MaskedCrossEntropy" else crit(x, target)
        loss.backward()
        _close(f"{form['id']} C={C}", loss.detach(), x.grad, want, want_grad)
        # (M, C) rows take the same route
        if form["cls"] not in ("MaskedCrossEntropy", "Poly1FocalLoss"):
            rows = logits.transpose(1, 2).reshape(-1, C)
            assert torch.allclose(crit(rows, target.reshape(-1)), loss.detach(), rtol=1e-6, atol=0)


def test_the_oddities_are_visible_in_the_fixtures(golden):
    """each kept oddity changes the recorded number by far more than the bounds above: the fixtures can tell"""
    C = 13
    by_id = {f["id"]: f for f in lf.forms(C)}
    logits, target, _ = lf.inputs(C, N)
    want = float(golden["focal_gamma2/C13/loss"])
    x = logits.double().requires_grad_(True)
    lp = torch.log_softmax(x.transpose(1, 2).reshape(-1, C), 1).gather(1, target.view(-1, 1)).view(-1)
    (-(1 - lp.exp()) ** 2 * lp).mean().backward()  # pt attached: same value, another gradient
    assert float((x.grad - torch.from_numpy(golden["focal_gamma2/C13/grad"]).double()).abs().max()) > 1e-5
    rows, y = logits.double().transpose(1, 2).reshape(-1, C), target.reshape(-1)
    weighted_mean = (torch.nn.functional.cross_entropy(rows, y, weight=torch.from_numpy(lf.class_weights(C)))  # torch's: / sum w[y]
                     + (1 - torch.softmax(rows, 1).gather(1, y.view(-1, 1))).mean())
    assert abs(float(weighted_mean) - float(golden["poly1ce_weight/C13/loss"])) > 1e-3
    torch_rule = dict(by_id["masked"], kwargs={})  # eps / C over everything, no mask: not SmoothCrossEntropy's rule
    other, _ = lf.evaluate(torch_rule, logits, target, torch.ones_like(target))
    assert abs(float(other) - float(golden["smooth_default/C13/loss"])) > 1e-3 and np.isfinite(want)


def test_multi_shape_and_the_classification_criteria(golden):
    shapes = [torch.from_numpy(golden[f"multishape/logits{i}"]) for i in range(2)]
    points, shape_labels = torch.from_numpy(golden["multishape/points"]), torch.from_numpy(golden["multishape/shape_labels"])
    for route in ("restatement", "product"):
        if route == "product":
            xs = [s.clone().requires_grad_(True) for s in shapes]
            loss = _build("MultiShapeCrossEntropy", criterion_args={"NAME": "SmoothCrossEntropy"})(xs, points, shape_labels)
        else:
            xs = [s.double().requires_grad_(True) for s in shapes]
            loss = lf.multi_shape(lf.smooth_cross_entropy, xs, points, shape_labels)
        loss.backward()
        for i in range(2):
            _close(f"multishape {route} shape {i}", loss.detach(), xs[i].grad, float(golden["multishape/loss"]),
                   torch.from_numpy(golden[f"multishape/grad{i}"]).double())
    rows = torch.from_numpy(golden["classification/rows"])
    for name, fn in (("LabelSmoothingCrossEntropy", lf.label_smoothing_ce), ("SoftTargetCrossEntropy", lf.soft_target_ce)):
        tgt = torch.from_numpy(golden[name + "/target"])
        want, want_grad = float(golden[name + "/loss"]), torch.from_numpy(golden[name + "/grad"]).double()
        x = rows.double().requires_grad_(True)
        loss = fn(x, tgt)
        loss.backward()
        _close(name + " restatement", loss.detach(), x.grad, want, want_grad)
        x = rows.clone().requires_grad_(True)
        loss = _build(name)(x, tgt)
        loss.backward()
        _close(name + " product", loss.detach(), x.grad, want, want_grad)


def test_weights_follow_the_logits_and_other_inputs_take_the_composition():
    """numpy and list weights become fp32 tensors; float64 logits, return_valid and reduction='none' stay on torch"""
    C = 13
    logits, target, _ = lf.inputs(C, 64)
    crit = _build("SmoothCrossEntropy", weight=list(lf.class_weights(C)), return_valid=True)
    assert crit.weight.dtype == torch.float32
    loss, pred, gt = crit(logits, target)
    assert pred.shape == (2 * 64, C) and gt.shape == (2 * 64,) and torch.isfinite(loss)
    per_point = _build("Poly1CrossEntropyLoss", num_classes=C, reduction="none")(logits, target)
    assert per_point.shape == (2 * 64,)
    assert abs(float(per_point.mean()) - float(_build("Poly1CrossEntropyLoss", num_classes=C)(logits, target))) < 1e-6
    per_element = _build("Poly1FocalLoss", reduction="none")(logits, target)
    assert per_element.shape == (2, C, 64)
    assert _build("FocalLoss", gamma=2)(logits.double(), target).dtype == torch.float64
