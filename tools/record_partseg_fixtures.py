"""Records what the reference's own part-segmentation classes compute on the CPU (models/segmentation/base_seg.py BasePartSeg
and MultiSegHead, models/backbone/pointnext.py PointNextPartDecoder, models/backbone/pointnetv2.py PointNet2PartDecoder):

    python tools/record_partseg_fixtures.py   (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/partseg.npz              3 clouds of 512 points in [0, 0.7]^3 with seven feature channels and three different
                                        shape categories; width 8, nsample 16, 50 part classes, no dropout.  Per variant --
                                        'pointnet2', 'curvenet', 'pointnext', 'pointnext1' (PointNeXt-S at strides [1,2,2,2,2],
                                        sa_layers 3, one per cls_map), 'blocks' (cls_map pointnet2 with decoder_blocks
                                        [2,2,1,1]: an InvResMLP block behind each of the two finest FP modules), 'pn2'
                                        (PointNet++ with PointNet2PartDecoder, width 4) -- the initial state dict, the logits
                                        in eval and train mode at every LOGIT_STRIDE-th point, the loss logits.square().mean()
                                        over ALL logits in both modes, the gradients of the first and last conv weight, of
                                        the class-conditioned FP conv and of convc / global_conv*, and the largest deviation
                                        of the fp32 logits, loss and gradients from the same step in fp64.  A tensor whose
                                        key and shape an earlier variant has starts from that variant's values and is stored
                                        once, as sd::<key>::<shape>; gradients of more than 4096 numbers keep every 8th row.
                                        'multi': the 'pointnet2' model with MultiSegHead -- state dict, part labels, the
                                        MultiShapeCrossEntropy value in eval and train mode and the gradient of one head.
  tests/golden/partseg_state_keys.json  state-dict keys and shapes per variant, in order

Only numbers are written: nothing of the reference's program text.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refshim import load_reference  # noqa: E402

load_reference()
from openpoints.loss import build_criterion_from_cfg  # noqa: E402  (the reference's)
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.models.layers import group as G  # noqa: E402
from openpoints.models.layers import upsampling as U  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

from amcontrast3d_amd import configs  # noqa: E402  (plain dicts; imports nothing of the drop-in package)

B, N, SIDE, RADIUS, NSAMPLE, CLASSES, LOGIT_STRIDE = 3, 512, 0.7, 0.1, 16, 50, 32
SHAPES = [3, 10, 15]  # 4, 6 and 3 parts
VARIANTS = {"pointnet2": ("pointnext-s", 8, {"cls_map": "pointnet2"}), "curvenet": ("pointnext-s", 8, {"cls_map": "curvenet"}),
            "pointnext": ("pointnext-s", 8, {"cls_map": "pointnext"}), "pointnext1": ("pointnext-s", 8, {"cls_map": "pointnext1"}),
            "blocks": ("pointnext-s", 8, {"cls_map": "pointnet2", "decoder_blocks": [2, 2, 1, 1]}),
            "pn2": ("pointnet++", 4, {}),
            "multi": ("pointnext-s", 8, {"cls_map": "pointnet2", "head": "MultiSegHead"})}

rng = np.random.default_rng(23)
pos = torch.from_numpy(rng.uniform(0, SIDE, (B, N, 3)).astype(np.float32))
extra = rng.uniform(-1, 1, (B, N, 4)).astype(np.float32)
x = torch.from_numpy(np.concatenate([pos.numpy(), extra], axis=-1).transpose(0, 2, 1).copy())
cls = torch.tensor(SHAPES, dtype=torch.int64).reshape(B, 1)
parts = torch.from_numpy(np.stack([rng.integers(0, configs.SHAPENETPART_NUM_PARTS[s], N) for s in SHAPES]))  # labels inside a shape
out = {"pos": pos.numpy(), "x": x.numpy(), "cls": cls.numpy(), "parts": parts.numpy().astype(np.int16),
       "meta": np.array([B, N, NSAMPLE, CLASSES, LOGIT_STRIDE]), "radius": np.array(RADIUS)}
keys = {}


def fixture_cfg(tag):
    variant, width, kw = VARIANTS[tag]
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_partseg(variant, num_classes=CLASSES, dropout=0, radius=RADIUS, nsample=NSAMPLE, width=width,
                                         global_feat=None, **kw))
    return cfg


def recorded_grads(model):
    """first and last conv weight, the class-conditioned FP conv, convc / global_conv*"""
    names = [k for k, p in model.named_parameters() if p.dim() >= 2]
    pick = [names[0], names[-1]]
    pick.append("decoder.FP_modules.0.convs.0.0.weight" if hasattr(model.decoder, "FP_modules") else "decoder.decoder.0.0.convs.0.0.weight")
    pick += [k for k in names if k.startswith(("decoder.convc.", "decoder.global_conv"))]
    return pick


def _gather_group(features, idx):
    """grouping_operation in plain torch, for any dtype (the shimmed operators take fp32 only)"""
    b, c = features.shape[:2]
    return features.gather(2, idx.reshape(b, 1, -1).expand(-1, c, -1).long()).reshape(b, c, *idx.shape[1:])


def _gather_interpolate(features, idx, weight):
    return (_gather_group(features, idx) * weight.unsqueeze(1).to(features.dtype)).sum(-1)


class fp64_operators:
    """the two feature-carrying operators of the shim replaced by dtype-agnostic torch for the fp64 twin"""

    def __enter__(self):
        self.keep = (G.grouping_operation, U.three_interpolate)
        G.grouping_operation, U.three_interpolate = _gather_group, _gather_interpolate

    def __exit__(self, *exc):
        G.grouping_operation, U.three_interpolate = self.keep


def double_twin(model):
    """the same model in fp64; the fp32 one-hot / part-table rows entering convc are cast on the way in"""
    twin = copy.deepcopy(model).double()
    if hasattr(twin.decoder, "convc"):
        twin.decoder.convc.register_forward_pre_hook(lambda m, a: (a[0].double(),))
    if getattr(twin.decoder, "cls2partembed", None) is not None:
        twin.decoder.cls2partembed = twin.decoder.cls2partembed.double()
    return twin


def batch(double=False):
    return {"pos": pos.clone(), "x": x.double() if double else x.clone(), "cls": cls.clone()}


def train_step(model, data, loss_of):
    model.train()
    model.zero_grad()
    logits = model(data)
    loss = loss_of(logits)
    loss.backward()
    return logits, loss.detach()


def sd_key(k, shape):
    return "sd::%s::%s" % (k, "x".join(str(int(d)) for d in shape))


def share_and_store_state(tag, model):
    """a tensor whose key and shape an earlier variant already has takes that variant's values (the initial state is
    arbitrary; this keeps the file small): one array per (key, shape), whichever variants hold it"""
    sd = model.state_dict()
    keys[tag] = [[k, list(v.shape)] for k, v in sd.items()]
    with torch.no_grad():
        for k, v in sd.items():
            name = sd_key(k, v.shape)
            if name in out:
                v.copy_(torch.from_numpy(out[name]))
            else:
                out[name] = v.detach().clone().numpy()


def thinned(g):
    """gradients of the wide global_conv weights: every 8th row"""
    return g[::8] if g.size > 4096 else g


for tag in VARIANTS:
    torch.manual_seed(7)
    model = build_model_from_cfg(fixture_cfg(tag))
    share_and_store_state(tag, model)
    if tag == "multi":
        cc = EasyConfig()
        cc.update({"NAME": "MultiShapeCrossEntropy", "criterion_args": {"NAME": "CrossEntropy"}})
        crit = build_criterion_from_cfg(cc)
        loss_of = lambda logits: crit(logits, parts, cls.reshape(-1))  # noqa: E731
        model.eval()
        with torch.no_grad():
            out["multi_loss_eval"] = loss_of(model(batch())).numpy()
        logits, loss = train_step(model, batch(), loss_of)
        assert len(logits) == 16 and [t.shape[1] for t in logits] == configs.SHAPENETPART_NUM_PARTS
        out["multi_loss"] = loss.numpy()
        head = f"head.multi_shape_heads.{SHAPES[1]}.0.0.weight"
        out["multi_grad_names"] = np.array([head])
        out[f"multi_grad::{head}"] = dict(model.named_parameters())[head].grad.numpy()
        print("multi: MultiShapeCrossEntropy", float(out["multi_loss_eval"]), "(eval)", float(loss), "(train)")
        continue
    out[f"{tag}_channel_list"] = np.array(model.encoder.channel_list)
    out[f"{tag}_out_channels"] = np.array(model.decoder.out_channels)
    square = lambda logits: logits.square().mean()  # noqa: E731
    model.eval()
    with torch.no_grad():
        ev = model(batch())
    out[f"{tag}_logits_eval"] = ev[:, :, ::LOGIT_STRIDE].numpy()
    out[f"{tag}_loss_eval"] = square(ev).numpy()
    out[f"{tag}_logits_range"] = np.array([float(ev.abs().max())])
    twin = double_twin(model)  # the same step in fp64: what the fp32 arithmetic alone costs
    logits, loss = train_step(model, batch(), square)
    logits = logits.detach()
    out[f"{tag}_logits_train"] = logits[:, :, ::LOGIT_STRIDE].numpy()
    out[f"{tag}_logits_range"] = np.array([float(ev.abs().max()), float(logits.abs().max())])
    out[f"{tag}_loss"] = loss.numpy()
    picks = recorded_grads(model)
    out[f"{tag}_grad_names"] = np.array(picks)
    grads = dict(model.named_parameters())
    for k in picks:
        out[f"{tag}_grad::{k}"] = thinned(grads[k].grad.numpy())
    with fp64_operators():
        logits64, loss64 = train_step(twin, batch(True), square)
    dev = {"logits": float((logits.double() - logits64.detach()).abs().max()), "loss": abs(float(loss) - float(loss64))}
    g64 = dict(twin.named_parameters())
    dev["grad"] = max(float((grads[k].grad.double() - g64[k].grad).abs().max() / g64[k].grad.abs().max()) for k in picks)
    out[f"{tag}_fp64_dev"] = np.array([dev["logits"], dev["loss"], dev["grad"]])
    print(tag, "fp32 against fp64: logits %.3e, loss %.3e, gradients %.3e of a tensor's range" % tuple(out[f"{tag}_fp64_dev"]),
          "| logits up to %.3f, loss %.6f" % (float(logits.abs().max()), float(loss)))

os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "partseg.npz"), **out)
with open(os.path.join(ROOT, "tests", "golden", "partseg_state_keys.json"), "w") as fh:
    json.dump(keys, fh, indent=0)
print("wrote", sum(v.nbytes for v in out.values()), "bytes of arrays;",
      os.path.getsize(os.path.join(ROOT, "tests", "golden", "partseg.npz")), "bytes compressed")
