"""Part segmentation end to end on synthetic shapes: BasePartSeg with the PointNeXt-S, PointNet++ or ASSANet encoder, a few
train steps and an evaluation pass, once per head:

    SegHead + CrossEntropy                 50 part logits per point, through train.train_one_epoch (its eager loop)
    MultiSegHead + MultiShapeCrossEntropy  one head per shape category, in a hand-written loop (the loss takes the shape labels)

    python examples/partseg_synthetic.py [--variant pointnext-s] [--cls-map curvenet] [--steps 8] [--batch 16] [--points 2048]

There are no datasets in this repository: a "shape" of category s is a union of num_parts[s] Gaussian blobs whose centres depend
on the category, a point's label is its blob, and its features are position, direction from the centroid and height (seven
channels, as ShapeNetPart's position + normal + height).  A model learns these within a few steps.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import configs, train  # noqa: E402
from openpoints.loss import build_criterion_from_cfg  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

NUM_PARTS = configs.SHAPENETPART_NUM_PARTS
FIRST_PART = np.concatenate([[0], np.cumsum(NUM_PARTS)])[:-1]
CENTRES = np.random.default_rng(0).uniform(0.15, 0.55, (16, max(NUM_PARTS), 3)).astype(np.float32)


def make_batch(batch, points, seed):
    """collated like the reference's ShapeNetPart batches: point-major 'pos', 'x' (direction + height), 'y' global part ids,
    'cls' (B,1) shape categories; 'y_local' are the part ids inside the shape (MultiShapeCrossEntropy's labels)"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 16, batch)
    local = np.stack([rng.integers(0, NUM_PARTS[s], points) for s in cls])
    pos = (CENTRES[cls[:, None], local] + 0.04 * rng.standard_normal((batch, points, 3))).astype(np.float32)
    away = pos - pos.mean(1, keepdims=True)
    away /= np.linalg.norm(away, axis=-1, keepdims=True) + 1e-6
    x = np.concatenate([away, pos[:, :, 2:3] - pos[:, :, 2:3].min(1, keepdims=True)], axis=-1).astype(np.float32)
    return {"pos": torch.from_numpy(pos), "x": torch.from_numpy(x), "cls": torch.from_numpy(cls.reshape(batch, 1)),
            "y": torch.from_numpy(local + FIRST_PART[cls][:, None]), "y_local": torch.from_numpy(local)}


def on_device(data, dev, feature_keys="pos,x"):
    data = {k: v.to(dev) for k, v in data.items()}
    data["x"] = train.get_features_by_keys(data, feature_keys)
    return data


def part_accuracy(logits, data):
    """share of points whose best part AMONG THE PARTS OF THEIR SHAPE is the labelled one"""
    hit = total = 0
    for b, s in enumerate(data["cls"].reshape(-1).tolist()):
        if isinstance(logits, list):
            pred = logits[s][b].argmax(0)
            hit += int((pred == data["y_local"][b]).sum())
        else:
            lo = int(FIRST_PART[s])
            pred = logits[b, lo:lo + NUM_PARTS[s]].argmax(0) + lo
            hit += int((pred == data["y"][b]).sum())
        total += pred.numel()
    return 100.0 * hit / total


def build(args, head, dev):
    kw = {"cls_map": args.cls_map} if args.variant == "pointnext-s" else {}
    c = EasyConfig()
    c.update(configs.model_cfg_partseg(args.variant, nsample=args.nsample, head=head, **kw))
    return build_model_from_cfg(c).to(dev)


def evaluate(model, args, dev):
    model.eval()
    with torch.no_grad():
        data = on_device(make_batch(args.batch, args.points, 999), dev)
        return part_accuracy(model(data), data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="pointnext-s", choices=["pointnext-s", "pointnet++", "assanet"])
    ap.add_argument("--cls-map", default="curvenet", choices=["pointnet2", "curvenet", "pointnext", "pointnext1"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--nsample", type=int, default=32)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    # branch 1: SegHead + CrossEntropy through train_one_epoch; the batch carries 'cls', the model reads it
    torch.manual_seed(0)
    model = build(args, "SegHead", dev)
    cc = EasyConfig(); cc.update({"NAME": "CrossEntropy"})
    criterion = build_criterion_from_cfg(cc).to(dev)
    cfg = EasyConfig()
    cfg.update({"num_classes": 50, "ignore_index": None, "feature_keys": "pos,x", "use_amp": False, "step_per_update": 1,
                "grad_norm_clip": 10, "sched_on_epoch": True, "criterion_args": {"NAME": "CrossEntropy"}})
    opt = torch.optim.AdamW(model.parameters(), lr=0.005, weight_decay=1e-4)
    loader = (make_batch(args.batch, args.points, 100 + k) for k in range(args.steps))
    out = train.train_one_epoch(model, loader, criterion, opt, None, None, 1, cfg)
    torch.cuda.synchronize()
    print(f"SegHead + CrossEntropy: {args.steps} steps, mean loss {out[0]:.3f}, train OA {out[3]:.1f} | "
          f"eval part accuracy {evaluate(model, args, dev):.1f} %")

    # branch 2: MultiSegHead + MultiShapeCrossEntropy: the criterion takes the shape labels, so the loop is written out
    torch.manual_seed(0)
    model = build(args, "MultiSegHead", dev)
    cc = EasyConfig(); cc.update({"NAME": "MultiShapeCrossEntropy", "criterion_args": {"NAME": "CrossEntropy"}})
    criterion = build_criterion_from_cfg(cc).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=0.005, weight_decay=1e-4)
    model.train()
    losses = []
    for k in range(args.steps):
        data = on_device(make_batch(args.batch, args.points, 100 + k), dev)
        opt.zero_grad()
        loss = criterion(model(data), data["y_local"], data["cls"].reshape(-1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10)
        opt.step()
        losses.append(float(loss.detach()))
    print(f"MultiSegHead + MultiShapeCrossEntropy: {args.steps} steps, loss {losses[0]:.3f} -> {losses[-1]:.3f} | "
          f"eval part accuracy {evaluate(model, args, dev):.1f} %")


if __name__ == "__main__":
    main()
