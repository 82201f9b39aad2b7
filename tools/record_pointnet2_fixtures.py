"""Records what the reference's own PointNet++ / ASSANet classes compute on the CPU (models/backbone/pointnetv2.py,
models/layers/local_aggregation.py):

    python tools/record_pointnet2_fixtures.py   (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/pointnet2.npz              per variant -- 'ssg', 'msg' (radii r and 2r per stage), 'assa' (ASSANet: stem conv and
                                          aggregation, query_as_support, residuals, blocks [2,2,2,2], mean, normalize_dp) --
                                          at 2 x 1024 points in [0, 0.7]^3, radius 0.1 doubling per stage, nsample 16, narrow
                                          widths: the initial state dict, logits in eval and train mode, the loss
                                          logits.square().mean(), the gradients of the first and last conv weight and of one
                                          BatchNorm weight per stage, channel_list / out_channels, and the largest deviation
                                          of the fp32 logits and gradients from the same model run in fp64;
                                          per stage and scale of 'msg' the ball-query rows and every query's in-radius count;
                                          one ASSA module on its own: its grouper's idx / dp, the features entering the
                                          aggregation and the tensor entering convs[num_preconv], for mean, sum and max
  tests/golden/pointnet2_state_keys.json  state-dict keys and shapes per variant, in order

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
from openpoints.models import build_model_from_cfg  # noqa: E402  (the reference's)
from openpoints.models.layers import group as G  # noqa: E402
from openpoints.models.layers import upsampling as U  # noqa: E402
from openpoints.models.layers.local_aggregation import LocalAggregation  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

from amcontrast3d_amd import configs  # noqa: E402  (plain dicts; imports nothing of the drop-in package)

B, N, SIDE, RADIUS, NSAMPLE = 2, 1024, 0.7, 0.1, 16
VARIANTS = {"ssg": ("pointnet++", 4), "msg": ("pointnet++msg", 4), "assa": ("assanet", 9)}
CLASSES = 5  # (logits are the bulk of the file: 2 x CLASSES x 1024 floats per variant and mode)

rng = np.random.default_rng(11)
pos = torch.from_numpy(rng.uniform(0, SIDE, (B, N, 3)).astype(np.float32))
colour = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
x = torch.from_numpy(np.concatenate([colour, pos.numpy()[:, :, 2:3]], axis=-1).transpose(0, 2, 1).copy())
out = {"pos": pos.numpy(), "x": x.numpy(), "meta": np.array([B, N, NSAMPLE]), "radius": np.array(RADIUS)}
keys = {}


def fixture_cfg(tag):
    variant, width = VARIANTS[tag]
    cfg = EasyConfig()
    cfg.update(configs.model_cfg_pointnet2(variant, num_classes=CLASSES, dropout=0, radius=RADIUS, nsample=NSAMPLE, width=width))
    return cfg


def recorded_grads(model):
    """first and last conv weight, the first BatchNorm weight of every SA module"""
    names = [k for k, p in model.named_parameters() if p.dim() >= 2]
    pick = [names[0], names[-1]]
    for s in range(len(model.encoder.SA_modules)):
        pick.append(next(k for k, p in model.named_parameters() if k.startswith(f"encoder.SA_modules.{s}.") and p.dim() == 1))
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


def train_step(model, data):
    model.train()
    model.zero_grad()
    logits = model(data)
    loss = logits.square().mean()
    loss.backward()
    return logits.detach(), loss.detach()


for tag in VARIANTS:
    torch.manual_seed(7)
    model = build_model_from_cfg(fixture_cfg(tag))
    sd = copy.deepcopy(model.state_dict())
    keys[tag] = [[k, list(v.shape)] for k, v in sd.items()]
    for k, v in sd.items():
        out[f"{tag}_sd::{k}"] = v.numpy()
    out[f"{tag}_channel_list"] = np.array(model.encoder.channel_list)
    out[f"{tag}_out_channels"] = np.array(model.encoder.out_channels)
    data = {"pos": pos.clone(), "x": x.clone()}
    model.eval()
    with torch.no_grad():
        out[f"{tag}_logits_eval"] = model(dict(data)).numpy()
    twin = copy.deepcopy(model).double()  # the same step in fp64: what the fp32 arithmetic alone costs
    logits, loss = train_step(model, dict(data))
    out[f"{tag}_logits_train"] = logits.numpy()
    out[f"{tag}_loss"] = loss.numpy()
    picks = recorded_grads(model)
    out[f"{tag}_grad_names"] = np.array(picks)
    grads = dict(model.named_parameters())
    for k in picks:
        out[f"{tag}_grad::{k}"] = grads[k].grad.numpy()
    with fp64_operators():
        logits64, loss64 = train_step(twin, {"pos": pos.clone(), "x": x.double()})
    dev = {"logits": float((logits.double() - logits64).abs().max()), "loss": abs(float(loss) - float(loss64))}
    g64 = dict(twin.named_parameters())
    dev["grad"] = max(float((grads[k].grad.double() - g64[k].grad).abs().max() / g64[k].grad.abs().max()) for k in picks)
    out[f"{tag}_fp64_dev"] = np.array([dev["logits"], dev["loss"], dev["grad"]])
    print(tag, "fp32 against fp64: logits %.3e, loss %.3e, gradients %.3e of a tensor's range" % tuple(out[f"{tag}_fp64_dev"]))

    if tag == "msg":  # the ball-query rows of every stage and scale, and how many points each query has in its radius
        clouds = model.encoder.forward_seg_feat(pos.clone(), x.clone())[0]
        for s, sa in enumerate(model.encoder.SA_modules):
            sup, qry = clouds[s], clouds[s + 1]
            d2 = ((qry[:, :, None, :] - sup[:, None, :, :]) ** 2).sum(-1)
            for j, la in enumerate(sa.local_aggregations):
                grouper = la.SA_CONFIG_operator.grouper
                idx = G.ball_query(grouper.radius, grouper.nsample, sup.contiguous(), qry.contiguous())
                out[f"cover_idx_{s}_{j}"] = idx.numpy().astype(np.int16)
                out[f"cover_cnt_{s}_{j}"] = (d2 < grouper.radius ** 2).sum(-1).numpy().astype(np.int16)
                out[f"cover_radius_{s}_{j}"] = np.array(grouper.radius)

# one ASSA module on its own: 300 support points, 77 queries, C' = ceil(16 / 3) = 6
M1, N1 = 77, 300
sup = torch.from_numpy(rng.uniform(0, 0.5, (B, N1, 3)).astype(np.float32))
pick = torch.from_numpy(np.stack([rng.permutation(N1)[:M1] for _ in range(B)]))
qry = torch.gather(sup, 1, pick.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
feat = torch.from_numpy(rng.standard_normal((B, 10, N1)).astype(np.float32))
out.update({"one_sup": sup.numpy(), "one_qry": qry.numpy(), "one_feat": feat.numpy(), "one_pick": pick.numpy()})
for reduction in ("mean", "sum", "max"):
    torch.manual_seed(3)
    args = EasyConfig()
    args.update({"aggr": {"NAME": "ASSA", "feature_type": "assa", "reduction": reduction},
                 "group": {"NAME": "ballquery", "radius": 0.12, "nsample": 16, "normalize_dp": True},
                 "conv": {"order": "conv-norm-act"}, "norm": {"norm": "bn"}, "act": {"act": "relu"}})
    la = LocalAggregation([10, 16, 16, 16], args.aggr, args.conv, args.norm, args.act, args.group, True).train()
    op = la.SA_CONFIG_operator
    seen = {}
    op.convs[op.num_preconv].register_forward_pre_hook(lambda m, a: seen.__setitem__("agg", a[0].detach().clone()))
    op.grouper.register_forward_hook(lambda m, a, r: seen.update(dp=r[0].detach().clone(), f=a[2].detach().clone()))
    la(qry, sup, feat, pick)
    out[f"one_{reduction}_agg"] = seen["agg"].numpy()
    if reduction == "mean":
        out["one_idx"] = G.ball_query(0.12, 16, sup, qry).numpy().astype(np.int32)
        out["one_dp"] = seen["dp"].numpy()
        out["one_f"] = seen["f"].numpy()  # the pre-convolved features the aggregation gathers from
    else:
        assert np.array_equal(out["one_dp"], seen["dp"].numpy()) and np.array_equal(out["one_f"], seen["f"].numpy())

os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pointnet2.npz"), **out)
with open(os.path.join(ROOT, "tests", "golden", "pointnet2_state_keys.json"), "w") as fh:
    json.dump(keys, fh, indent=0)
print("wrote", sum(v.nbytes for v in out.values()), "bytes of arrays;",
      os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet2.npz")), "bytes compressed")
