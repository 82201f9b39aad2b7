"""Cost of ScanNet's training input on the device (input_pipeline.scannet_train_batch: ScanNet.__getitem__ of
dataset/scannetv2/scannet.py:140-176 for two raw rooms plus the collate) next to the numpy restatement of the same chain on
the host (tests/scannet_input_ref.py, one room after the other, as one loader worker would):

    python tools/scannet_input_bench.py [reps=20]  -> one JSON line

A batch is cfg 4's: 2 raw rooms of ~157 k points each, voxelised at 2 cm, cropped to 64000 points.  Device time is wall
clock per batch with the GPU synchronised at the end (the per-room voxel-count read-backs are inside it)."""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from amcontrast3d_amd import input_pipeline  # noqa: E402
from amcontrast3d_amd.augment import ScanNetTrainAugment  # noqa: E402
import scannet_input_ref as ref  # noqa: E402

KWARGS = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
          "color_mean": list(ref.COLOR_MEAN), "color_std": list(ref.COLOR_STD)}


def room(seed, side=280, spacing=0.022):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * spacing
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 0.8], len(g))
    base = np.concatenate([g, z[:, None]], 1) + np.array([-3.0, 1.0, 0.2])
    coord = np.concatenate([base + rng.uniform(-0.003, 0.003, base.shape) for _ in range(2)], 0).astype(np.float32)
    return coord, rng.uniform(-1, 1, coord.shape).astype(np.float32), rng.integers(0, 20, len(coord)).astype(np.int64)


def host_item(coord, feat, label, rng):
    """the restatement with numpy's own draws, in the reference's order"""
    a = rng.uniform(-math.pi, math.pi)
    pos, x = ref.transform_room(coord, feat, ref.rotation(a), rng.uniform(0.8, 1.2), rng.random(3), rng.random(), rng.random(),
                                rng.random())
    key = ref.fnv_hash_vec(np.floor((pos - pos.min(0)) / np.array(0.02)))
    count = np.unique(key, return_counts=True)[1]
    n = len(count)
    return ref.crop_room(pos, x, label, 0.02, 64000, False, rng.integers(0, count.max(), n), int(rng.integers(n)),
                         None, rng.permutation(64000))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    rooms = [room(1), room(2)]
    g = [tuple(torch.from_numpy(a).to(dev) for a in r) for r in rooms]
    aug = ScanNetTrainAugment(**KWARGS)
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(3):
        out = input_pipeline.scannet_train_batch(g, aug, 0.02, 64000, generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = input_pipeline.scannet_train_batch(g, aug, 0.02, 64000, generator=gen)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    rng = np.random.default_rng(0)
    host_item(*rooms[0], rng)
    t0 = time.perf_counter()
    host_reps = 3
    for _ in range(host_reps):
        for r in rooms:
            host_item(*r, rng)
    dh = (time.perf_counter() - t0) / host_reps
    print(json.dumps({"metric": "ScanNet training input per 2-room batch (transforms + fp64 voxelise 2 cm + crop to 64000 + "
                                "collate)", "device_ms_per_batch": round(dt * 1e3, 3), "host_numpy_ms_per_batch": round(dh * 1e3, 1),
                      "raw_points_per_room": [len(r[0]) for r in rooms], "batch_shape": list(out["pos"].shape), "reps": reps}))


if __name__ == "__main__":
    main()
