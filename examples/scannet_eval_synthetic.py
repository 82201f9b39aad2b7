"""Validation and whole-room testing of a synthetic ScanNet-style raw room on the device route: the plain PointNeXt baseline
built from the keys of cfgs/scannet/pointnext-xl.yaml, the multi-step schedule of cfgs/scannet/default.yaml, the val item of
ScanNet.__getitem__ (`input_pipeline.scannet_val_cloud` -> `evaluate.validate_boundary_inner`) and the test loop
(`evaluate.test_room_scannet`: sub-clouds, model batches and the vote on the GPU), ending with the benchmark's label ids.

    python examples/scannet_eval_synthetic.py [--points 150000] [--width 32] [--batch 4]

There are no datasets in this repository: the room is a jittered grid with random colours and labels, so the numbers mean
nothing; the shapes, the route and the reproducible vote are what it shows.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import evaluate, input_pipeline  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.scheduler import build_scheduler_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402


def raw_room(points, seed=0, spacing=0.022):
    """what torch.load of a ScanNet .pth gives: coord (n,3) fp32, colours in [-1, 1], labels 0..19 with -100"""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(points / 2))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * spacing
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 0.8], len(g))
    base = np.concatenate([g, z[:, None]], 1) + np.array([-3.0, 1.0, 0.2])
    coord = np.concatenate([base + rng.uniform(-0.003, 0.003, base.shape) for _ in range(2)], 0).astype(np.float32)
    label = rng.integers(0, 20, len(coord)).astype(np.int64)
    label[rng.random(len(label)) < 0.05] = -100
    return coord, rng.uniform(-1, 1, coord.shape).astype(np.float32), label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = EasyConfig()
    cfg.update({"model": {
        "NAME": "BaseSeg",
        "encoder_args": {"NAME": "PointNextEncoder", "blocks": [1, 1, 1, 1, 1], "strides": [1, 4, 4, 4, 4], "sa_layers": 1,
                         "sa_use_res": False, "width": args.width, "in_channels": 7, "expansion": 4, "radius": 0.05, "nsample": 32,
                         "aggr_args": {"feature_type": "dp_fj", "reduction": "max"},
                         "group_args": {"NAME": "ballquery", "normalize_dp": True},
                         "conv_args": {"order": "conv-norm-act"}, "act_args": {"act": "relu"}, "norm_args": {"norm": "bn"}},
        "decoder_args": {"NAME": "PointNextDecoder"},
        "cls_args": {"NAME": "SegHead", "num_classes": 20, "in_channels": None, "norm_args": {"norm": "bn"}, "global_feat": "max"}},
        # cfgs/scannet/default.yaml:70-81
        "lr": 0.001, "epochs": 100, "sched": "multistep", "decay_epochs": [70, 90], "decay_rate": 0.1, "warmup_epochs": 0,
        "feature_keys": "pos,x,heights", "num_classes": 20, "ignore_index": -100})
    model = build_model_from_cfg(cfg.model).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=cfg.lr)
    sched = build_scheduler_from_cfg(cfg, opt)
    lrs = []
    for epoch in (1, 68, 69, 89):
        sched.step(epoch)
        lrs.append(f"{epoch}: {opt.param_groups[0]['lr']:.0e}")
    print("multi-step schedule, lr set at the end of epoch", ", ".join(lrs))

    coord, feat, label = raw_room(args.points)
    gen = torch.Generator(device=dev).manual_seed(0)
    room = tuple(torch.from_numpy(a).to(dev) for a in (coord, feat, label))
    val = input_pipeline.scannet_val_cloud(room, 0.02, generator=gen, feature_keys=cfg.feature_keys)
    v = evaluate.validate_boundary_inner(model, [val], cfg.num_classes, cfg.ignore_index, 16, miou_B_I=False)
    print(f"val item: {val['pos'].shape[1]} of {len(coord)} points, input {tuple(val['x'].shape)} | mIoU {v[0]:.1f} OA {v[2]:.1f}")

    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = evaluate.test_room_scannet(model, coord, feat, label, 0.02, cfg.num_classes, cfg.ignore_index, 16,
                                   feature_keys=cfg.feature_keys, miou_B_I=True, batch=args.batch,
                                   generator=torch.Generator(device=dev).manual_seed(1))
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    again = evaluate.test_room_scannet(model, coord, feat, None, 0.02, cfg.num_classes, cfg.ignore_index, 16,
                                       feature_keys=cfg.feature_keys, batch=args.batch,
                                       generator=torch.Generator(device=dev).manual_seed(1))
    s = evaluate.summarize(r["cm"], r["cm_b"], r["cm_i"])
    same = torch.equal(r["logits"].view(torch.int32), again["logits"].view(torch.int32))
    print(f"whole room ({len(coord)} points, {dt:.3f} s): mIoU {s[0]:.1f} OA {s[2]:.1f} boundary mIoU {s[5]:.1f} | "
          f"voted logits of a second run identical bit for bit: {same}")
    ids = evaluate.scannet_benchmark_ids(again["pred"])
    print("benchmark label ids of the first points:", ids[:10].tolist())


if __name__ == "__main__":
    main()
