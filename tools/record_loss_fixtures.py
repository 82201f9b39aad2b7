"""Records what the reference's own openpoints.loss classes compute, on the CPU, for the forms tests/loss_family_ref.py lists:

    python tools/record_loss_fixtures.py        (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/loss_family.npz               inputs, loss values and logit gradients at B = 2, N = 257: every form at C = 13, and
                                             at C = 20 the forms in AT_20 (one per way the class count enters a formula; all
                                             forms at both counts would pass the size limit for a committed file)
  tests/golden/loss_family_signatures.json   constructor and forward parameter names and defaults of each class

Only numbers and names are written: nothing of the reference's program text.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refshim import load_reference  # noqa: E402

load_reference()
import loss_family_ref as lf  # noqa: E402
from openpoints.loss import build_criterion_from_cfg  # noqa: E402  (the reference's)
from openpoints.loss.build import LOSS  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

B, N = 2, 257
AT_20 = ("smooth_default", "smooth_ignore3", "smooth_weight", "masked", "bce", "focal_alpha", "poly1ce_weight", "poly1focal_default")
CLASSES = ("SmoothCrossEntropy", "MaskedCrossEntropy", "BCELogits", "FocalLoss", "Poly1CrossEntropyLoss", "Poly1FocalLoss",
           "MultiShapeCrossEntropy", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy")


def build(name, kwargs):
    cfg = EasyConfig()
    cfg.update(dict(kwargs, NAME=name))
    return build_criterion_from_cfg(cfg)


def value_and_grads(crit, leaves, *rest):
    leaves = [x.clone().requires_grad_(True) for x in leaves]
    loss = crit(*(leaves if len(leaves) == 1 else [leaves]), *rest)
    loss.backward()
    return np.float32(loss.item()), [x.grad.numpy() for x in leaves]


out = {}
for C in (13, 20):
    for form in lf.forms(C):
        if C == 20 and form["id"] not in AT_20:
            continue
        logits, target, mask = lf.inputs(C, N, form["labels"], B)
        rest = (target, mask) if form["cls"] == "MaskedCrossEntropy" else (target,)
        loss, (grad,) = value_and_grads(build(form["cls"], form["kwargs"]), [logits], *rest)
        key = f"{form['id']}/C{C}"
        out[key + "/loss"], out[key + "/grad"] = loss, grad
        # the inputs are lf.inputs(C, N, labels): recorded once per label rule, so that a change of the generator shows
        out[f"inputs/{form['labels']}/C{C}/logits"], out[f"inputs/{form['labels']}/C{C}/target"] = logits.numpy(), target.numpy()
        out[f"inputs/{form['labels']}/C{C}/mask"] = mask.numpy()

# MultiShapeCrossEntropy over two shapes (13 and 4 part classes), SmoothCrossEntropy inside
g = torch.Generator().manual_seed(5)
shapes = [torch.randn(B, 13, N, generator=g) * 3, torch.randn(B, 4, N, generator=g) * 3]
shape_labels = torch.tensor([1, 0])
points = torch.stack([torch.randint(0, 4, (N,), generator=g), torch.randint(0, 13, (N,), generator=g)])
loss, grads = value_and_grads(build("MultiShapeCrossEntropy", {"criterion_args": {"NAME": "SmoothCrossEntropy"}}), shapes, points, shape_labels)
out.update({"multishape/logits0": shapes[0].numpy(), "multishape/logits1": shapes[1].numpy(), "multishape/points": points.numpy(),
            "multishape/shape_labels": shape_labels.numpy(), "multishape/loss": loss, "multishape/grad0": grads[0], "multishape/grad1": grads[1]})

# the classification criteria, on (M, C) rows
rows = torch.randn(64, 15, generator=g) * 3
labels = torch.randint(0, 15, (64,), generator=g)
soft = torch.softmax(torch.randn(64, 15, generator=g), dim=1)
for name, kwargs, tgt in (("LabelSmoothingCrossEntropy", {}, labels), ("SoftTargetCrossEntropy", {}, soft)):
    loss, (grad,) = value_and_grads(build(name, kwargs), [rows], tgt)
    out.update({f"{name}/loss": loss, f"{name}/grad": grad, f"{name}/target": tgt.numpy()})
out["classification/rows"] = rows.numpy()

golden = os.path.join(ROOT, "tests", "golden")
np.savez_compressed(os.path.join(golden, "loss_family.npz"), **out)


def parameters(fn):
    return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), p.kind.name]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


sig = {name: {"init": parameters(LOSS.module_dict[name].__init__), "forward": parameters(LOSS.module_dict[name].forward)}
       for name in CLASSES}
with open(os.path.join(golden, "loss_family_signatures.json"), "w") as f:
    json.dump(sig, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(out)} arrays, {os.path.getsize(os.path.join(golden, 'loss_family.npz'))} bytes")
