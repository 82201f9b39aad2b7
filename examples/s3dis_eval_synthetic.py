"""Validation and whole-room testing of a synthetic S3DIS-style raw room on the device route: PointNeXt built from the keys of
cfgs/s3dis/pointnext-xl.yaml, the val item of S3DIS.__getitem__ (`input_pipeline.s3dis_val_cloud` ->
`evaluate.validate_boundary_inner`) and the test loop (`evaluate.test_room_s3dis`: sub-clouds, the config's evaluation
transforms [PointsToTensor, PointCloudXYZAlign, ChromaticNormalize], model batches and the vote on the GPU) in both test
modes, ending with the sum over rooms that 6-fold testing is.

    python examples/s3dis_eval_synthetic.py [--points 200000] [--width 32] [--batch 4]

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
from openpoints.utils import EasyConfig  # noqa: E402


def raw_room(points, seed=0, spacing=0.03, copies=4):
    """what np.load of an Area_*.npy gives: (n,7) float64, xyz in metres, rgb 0..255, label 0..12"""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(points / copies))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * spacing
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 1.2], len(g))
    base = np.concatenate([g, z[:, None]], 1) + np.array([12.0, -7.0, 0.1])
    coord = np.concatenate([base + rng.uniform(-0.012, 0.012, base.shape) for _ in range(copies)], 0)
    colour = rng.integers(0, 256, coord.shape).astype(np.float64)
    label = rng.integers(0, 13, (len(coord), 1)).astype(np.float64)
    return np.concatenate([coord, colour, label], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = EasyConfig()
    cfg.update({"model": {
        "NAME": "BaseSeg",
        "encoder_args": {"NAME": "PointNextEncoder", "blocks": [1, 1, 1, 1, 1], "strides": [1, 4, 4, 4, 4], "sa_layers": 1,
                         "sa_use_res": False, "width": args.width, "in_channels": 4, "expansion": 4, "radius": 0.1, "nsample": 32,
                         "aggr_args": {"feature_type": "dp_fj", "reduction": "max"},
                         "group_args": {"NAME": "ballquery", "normalize_dp": True},
                         "conv_args": {"order": "conv-norm-act"}, "act_args": {"act": "relu"}, "norm_args": {"norm": "bn"}},
        "decoder_args": {"NAME": "PointNextDecoder"},
        "cls_args": {"NAME": "SegHead", "num_classes": 13, "in_channels": None, "norm_args": {"norm": "bn"}}},
        # cfgs/s3dis/default.yaml
        "feature_keys": "x,heights", "num_classes": 13, "ignore_index": None, "voxel_size": 0.04})
    model = build_model_from_cfg(cfg.model).to(dev)

    rooms = [raw_room(args.points, seed) for seed in (0, 1)]
    val = input_pipeline.s3dis_val_cloud(torch.from_numpy(rooms[0]).to(dev), cfg.voxel_size,
                                         generator=torch.Generator(device=dev).manual_seed(0), feature_keys=cfg.feature_keys)
    v = evaluate.validate_boundary_inner(model, [val], cfg.num_classes, cfg.ignore_index, 16, miou_B_I=False)
    print(f"val item: {val['pos'].shape[1]} of {len(rooms[0])} points, input {tuple(val['x'].shape)}, centre "
          f"{[round(c, 3) for c in val['centre'][0].tolist()]} | mIoU {v[0]:.1f} OA {v[2]:.1f}")

    all_cm = evaluate._matrices(cfg.num_classes, cfg.ignore_index)[0]
    for k, cdata in enumerate(rooms):  # 6-fold testing: the same sum over the rooms of every area
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = evaluate.test_room_s3dis(model, cdata, cfg.voxel_size, cfg.num_classes, cfg.ignore_index, 16,
                                     feature_keys=cfg.feature_keys, miou_B_I=True, batch=args.batch,
                                     generator=torch.Generator(device=dev).manual_seed(1))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        again = evaluate.test_room_s3dis(model, cdata[:, :6], cfg.voxel_size, cfg.num_classes, cfg.ignore_index, 16,
                                         feature_keys=cfg.feature_keys, batch=args.batch,
                                         generator=torch.Generator(device=dev).manual_seed(1))
        s = evaluate.summarize(r["cm"], r["cm_b"], r["cm_i"])
        same = torch.equal(r["logits"].view(torch.int32), again["logits"].view(torch.int32))
        print(f"room {k} ({len(cdata)} points, {dt:.3f} s): mIoU {s[0]:.1f} OA {s[2]:.1f} boundary mIoU {s[5]:.1f} | "
              f"voted logits of a second run identical bit for bit: {same}")
        all_cm.value += r["cm"].value
    s = evaluate.summarize(all_cm)
    print(f"all rooms: mIoU {s[0]:.1f} mAcc {s[1]:.1f} OA {s[2]:.1f}")
    nn = evaluate.test_room_s3dis(model, rooms[0], cfg.voxel_size, cfg.num_classes, cfg.ignore_index, 16,
                                  feature_keys=cfg.feature_keys, test_mode="nearest_neighbor",
                                  generator=torch.Generator(device=dev).manual_seed(2))
    print(f"test_mode nearest_neighbor: one sub-cloud, OA {evaluate.summarize(nn['cm'])[2]:.1f}")


if __name__ == "__main__":
    main()
