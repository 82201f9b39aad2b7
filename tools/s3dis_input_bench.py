"""S3DIS training input for one batch of raw rooms, three ways, in one process:  python tools/s3dis_input_bench.py [rooms=8]
[points=1000000] -> one JSON line.

  batched     input_pipeline.s3dis_train_batch on the list of rooms (csrc/room_input.hip; includes the concatenation)
  feed        the same through input_pipeline.S3DISTrainFeed, which keeps the rooms concatenated: what an epoch pays per batch
  per_room    the route without it: S3DIS.__getitem__'s cast and shift in torch, input_pipeline.crop_pc per room, torch.stack,
              augment.S3DISTrainAugment
  numpy       tests/s3dis_input_ref.train_item on one host core, ONE room (the reference's arithmetic, stable sorts)

All device routes draw from a device generator, produce (rooms, 24000) clouds at voxel 0.04 m and are timed by a host clock
around `calls` calls that end in a device synchronise.  The routes alternate, `reps` windows each, after a warm-up of every
route; the line holds the median window and the smallest and largest (the spread)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amcontrast3d_amd import input_pipeline as ip  # noqa: E402
from amcontrast3d_amd.augment import S3DISTrainAugment  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
N_RAW = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000  # S3DIS's median room (s3dis.py:48)
VOXEL, VOXEL_MAX, REPS, CALLS = 0.04, 24000, 7, 50
dev = torch.device("cuda:0")


def make_room(seed, n):
    """an (n,7) float64 raw room: floor, ceiling and four walls of a 10 m x 8 m x 3 m box with 1 cm noise, a few points per
    4 cm voxel at a million points; colours 0..255, labels 0..12"""
    rng = np.random.default_rng(seed)
    w, d, h = 10.0 + rng.uniform(-1, 1), 8.0 + rng.uniform(-1, 1), 3.0
    areas = np.array([w * d, w * d, w * h, w * h, d * h, d * h])
    face = rng.choice(6, n, p=areas / areas.sum())
    u, v = rng.random(n), rng.random(n)
    xyz = np.empty((n, 3))
    for f, (x, y, z) in enumerate(((u * w, v * d, 0 * u), (u * w, v * d, 0 * u + h), (u * w, 0 * u, v * h), (u * w, 0 * u + d, v * h),
                                   (0 * u, u * d, v * h), (0 * u + w, u * d, v * h))):
        m = face == f
        xyz[m] = np.stack([x[m], y[m], z[m]], 1)
    xyz += rng.normal(0, 0.01, xyz.shape) + np.array([-14.0, 22.0, 0.5])
    return np.concatenate([xyz, rng.integers(0, 256, (n, 3)).astype(np.float64), face[:, None].astype(np.float64)], 1)


rooms_np = [make_room(100 + b, N_RAW) for b in range(B)]
rooms = [torch.from_numpy(r).to(dev) for r in rooms_np]
aug = S3DISTrainAugment(color_drop=0.2, gravity_dim=2, scale=[0.9, 1.1], angle=[0, 0, 1], jitter_sigma=0.005, jitter_clip=0.02)
gen = torch.Generator(device=dev).manual_seed(0)
feed = ip.S3DISTrainFeed(rooms, aug, batch_size=B, voxel_size=VOXEL, voxel_max=VOXEL_MAX, generator=gen)


def batched():
    return ip.s3dis_train_batch(rooms, aug, VOXEL, VOXEL_MAX, generator=gen)


def from_feed():
    return next(iter(feed))


def per_room():
    pos, col, ys = [], [], []
    for room in rooms:
        cd = room.float()
        coord = cd[:, :3] - cd[:, :3].min(0).values
        c, f, l = ip.crop_pc(coord, cd[:, 3:6], cd[:, 6], "train", VOXEL, VOXEL_MAX, variable=False, generator=gen)
        pos.append(c), col.append(f), ys.append(l)
    p, x, h = aug(torch.stack(pos), torch.stack(col), generator=gen)
    return {"pos": p, "x": x, "heights": h, "y": torch.stack(ys)}


routes = {"batched": batched, "feed": from_feed, "per_room": per_room}
for fn in routes.values():
    for _ in range(2):
        out = fn()
    assert out["pos"].shape == (B, VOXEL_MAX, 3)
torch.cuda.synchronize()
windows = {k: [] for k in routes}
for _ in range(REPS):
    for k, fn in routes.items():
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        windows[k].append((time.perf_counter() - t0) / CALLS * 1e3)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


line = {"metric": "S3DIS training input, wall ms per batch of raw rooms -> (rooms, 24000) (voxel 0.04 m, device generator)",
        "rooms": B, "raw_points_per_room": N_RAW, "windows": REPS, "calls_per_window": CALLS}
line.update({k: stats(v) for k, v in windows.items()})
line["value"], line["unit"] = line["feed"]["median_ms"], "ms/batch"

import s3dis_input_ref as ref  # noqa: E402  (tools/: a measuring script, like bench.py's cpu_baseline leg)
from oracle import input_ref  # noqa: E402

torch.set_num_threads(1)
rng = np.random.default_rng(0)
c = rooms_np[0][:, :3].astype(np.float32)
count = np.unique(input_ref.fnv_hash_vec(np.floor((c - c.min(0)) / np.array(VOXEL))), return_counts=True)[1]
d = {"rnd": rng.integers(0, count.max(), len(count)), "init_idx": int(rng.integers(len(count))), "perm": rng.permutation(VOXEL_MAX),
     "contrast": True, "blend": 0.5, "scale_u": rng.random(3).astype(np.float32), "theta": np.array([0.0, 0.0, 1.0]),
     "noise": rng.standard_normal((VOXEL_MAX, 3)).astype(np.float32), "drop": False}
t0 = time.perf_counter()
ref.train_item(rooms_np[0], d, VOXEL, VOXEL_MAX)
line["numpy_one_room_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
line["voxels_room0"] = int(len(count))
print(json.dumps(line))
