"""Whole-room testing of one large S3DIS-sized room: the device route (evaluate.test_room_s3dis: room_parts, s3dis_part_batch,
the model, vote_parts) next to the host route (evaluate.voxel_parts on the host, evaluate.test_cloud_boundary_inner with a
host make_input that applies [PointsToTensor, PointCloudXYZAlign, ChromaticNormalize], scatter_mean):

    python tools/s3dis_eval_bench.py [--variants S] [--reps 3] [--warmup 1] [--batch 4] [--side 500]  -> one JSON line per variant

The room is synthetic: side * side * 4 raw float64 points (1 M by default), voxelised at 4 cm.  Times are wall clock per room
with the GPU synchronised at the end, the upload of the raw room included on both routes; median and min / max over the
repeats.  The split of the device route comes from a separate pass with a synchronisation after every phase (their sum
exceeds the unsplit time by the waits)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import amcontrast3d_amd  # noqa: E402

amcontrast3d_amd.activate()
from amcontrast3d_amd import evaluate, input_pipeline as ip, ops  # noqa: E402
from openpoints.models import build_model_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402

VARIANTS = {"XL": (64, [1, 4, 7, 4, 4]), "S": (32, [1, 1, 1, 1, 1])}
MEAN = np.array(ip.S3DIS_COLOR_MEAN).astype(np.float32)
STD = np.array(ip.S3DIS_COLOR_STD).astype(np.float32)
VOXEL, NCLS, IGNORE, NSAMPLE = 0.04, 13, None, 16


def room(seed, side, spacing=0.022, copies=4):
    """an Area_*.npy array: (n,7) float64, xyz, rgb 0..255, label"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * spacing
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 1.2], len(g))
    base = np.concatenate([g, z[:, None]], 1) + np.array([12.0, -7.0, 0.1])
    coord = np.concatenate([base + rng.uniform(-0.008, 0.008, base.shape) for _ in range(copies)], 0)
    colour = rng.integers(0, 256, coord.shape).astype(np.float64)
    label = rng.integers(0, NCLS, (len(coord), 1)).astype(np.float64)
    return np.concatenate([coord, colour, label], 1)


def model_cfg(variant):
    """the `model:` block of cfgs/s3dis/pointnext-xl.yaml (S: the standard PointNeXt-S widths under the same keys)"""
    width, blocks = VARIANTS[variant]
    return {"NAME": "BaseSeg",
            "encoder_args": {"NAME": "PointNextEncoder", "blocks": blocks, "strides": [1, 4, 4, 4, 4], "sa_layers": 1,
                             "sa_use_res": False, "width": width, "in_channels": 4, "expansion": 4, "radius": 0.1, "nsample": 32,
                             "aggr_args": {"feature_type": "dp_fj", "reduction": "max"},
                             "group_args": {"NAME": "ballquery", "normalize_dp": True},
                             "conv_args": {"order": "conv-norm-act"}, "act_args": {"act": "relu"}, "norm_args": {"norm": "bn"}},
            "decoder_args": {"NAME": "PointNextDecoder"},
            "cls_args": {"NAME": "SegHead", "num_classes": NCLS, "in_channels": None, "norm_args": {"norm": "bn"}}}


def host_route(model, cdata, batch, dev):
    """load_data's steps and the split on the host, the three transforms in make_input, one upload per sub-cloud"""
    t0 = time.perf_counter()
    coord, label = cdata[:, :3], cdata[:, 6]
    feat = np.clip(cdata[:, 3:6] / 255., 0, 1).astype(np.float32)
    shifted = coord - coord.min(0)
    parts = evaluate.voxel_parts(shifted, VOXEL, rng=np.random.default_rng(0))
    t_parts = time.perf_counter() - t0

    def make_input(coord_part, feat_part):
        heights = coord_part[:, 2:3].astype(np.float32)
        pos = torch.from_numpy(coord_part.astype(np.float32))
        pos -= torch.mean(pos, axis=0, keepdims=True)
        pos[:, 2] -= torch.min(pos[:, 2])
        x = feat_part
        if x.max() > 1:
            x = x / 255.
        x = (x - MEAN) / STD
        inp = np.ascontiguousarray(np.concatenate([x, heights], 1).T)
        return {"pos": pos.to(dev).unsqueeze(0), "x": torch.from_numpy(inp).to(dev).unsqueeze(0)}
    r = evaluate.test_cloud_boundary_inner(model, shifted, feat, torch.from_numpy(label.astype(np.int64)).to(dev), parts, NCLS,
                                           IGNORE, NSAMPLE, make_input=make_input, miou_B_I=False, batch=batch)
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0, t_parts, len(parts), len(parts[0])


def device_route(model, cdata, batch, gen):
    t0 = time.perf_counter()
    r = evaluate.test_room_s3dis(model, cdata, VOXEL, NCLS, IGNORE, NSAMPLE, batch=batch, generator=gen)
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


@torch.no_grad()
def device_split(model, cdata, batch, gen, dev):
    """test_room_s3dis's phases with a synchronisation after each"""
    out = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        out[name] = out.get(name, 0.0) + time.perf_counter() - t0
    t0 = time.perf_counter()
    d = torch.from_numpy(cdata).to(dev)
    c = d[:, :3] - d[:, :3].min(0).values
    f, y = d[:, 3:6].contiguous(), d[:, 6].long()
    lap("upload", t0)
    t0 = time.perf_counter()
    rp = ip.room_parts(c, VOXEL, generator=gen)
    lap("parts", t0)
    P, nvox = rp["parts"].shape
    logits = torch.empty(P, NCLS, nvox, device=dev)
    for j0 in range(0, P, batch):
        t0 = time.perf_counter()
        data = ip.s3dis_part_batch(rp["parts"][j0:j0 + batch], c, f, y, "test")
        lap("batch_assembly", t0)
        t0 = time.perf_counter()
        logits[j0:j0 + batch] = evaluate._logits(model(data))
        lap("model", t0)
    t0 = time.perf_counter()
    _, pred = ops.vote_parts(logits, rp)
    cm = evaluate._matrices(NCLS, IGNORE)[0]
    cm.update(pred, y)
    lap("vote", t0)
    return out, P, nvox


def stats(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="S")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--side", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cdata = room(1, args.side)
    for variant in args.variants.split(","):
        torch.manual_seed(0)
        c = EasyConfig()
        c.update(model_cfg(variant))
        model = build_model_from_cfg(c).to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(0)
        new, old, old_parts, split = [], [], [], []
        for k in range(args.warmup + args.reps):  # the routes alternate, so that drift hits both alike
            rn, tn = device_route(model, cdata, args.batch, gen)
            ro, to, tp, n_parts, n_vox = host_route(model, cdata, args.batch, dev)
            sp, P, nvox = device_split(model, cdata, args.batch, gen, dev)
            if k >= args.warmup:
                new.append(tn); old.append(to); old_parts.append(tp); split.append(sp)
        assert (P, nvox) == (n_parts, n_vox) and rn["pred"].shape == ro["pred"].shape
        print(json.dumps({"metric": "whole-room test of one S3DIS-sized room, PointNeXt-%s, %d sub-clouds of %d points, %d per "
                                    "model call" % (variant, P, nvox, args.batch),
                          "raw_points": len(cdata), "device_route": stats(new), "host_route": stats(old),
                          "host_route_parts_on_host": stats(old_parts),
                          "device_route_split_ms": {k: round(statistics.median(s[k] for s in split) * 1e3, 2) for k in split[0]},
                          "reps": args.reps, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
