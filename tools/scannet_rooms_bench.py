"""ScanNet training input for one batch of raw rooms, three ways, in one process:  python tools/scannet_rooms_bench.py [stages]
-> one JSON line.

  per_room    input_pipeline.scannet_train_batch: the transform for the batch, then voxelise / select / crop / tail room by room
  joint       input_pipeline.scannet_train_rooms on the list of rooms (csrc/room_input.hip; includes the concatenation)
  feed        input_pipeline.ScanNetTrainFeed on the same rooms kept resident: one epoch of `calls` batches per window, so the
              epoch's own two read-backs and the per-batch concatenation of the picked slices are in the figure

Two shapes: 2 rooms of 156800 points -> (2, 64000), the batch of cfgs/scannet/default.yaml, and 8 of the same rooms ->
(8, 32000), the smaller crop its comment mentions.  All routes draw from a device generator at voxel 0.02 m and are timed by a
host clock around `calls` calls that end in a device synchronise.  The routes alternate, `windows` windows each, after a
warm-up of every route; the line holds the median window and the smallest and largest (the spread).

With the argument `stages` every C entry point the routes call is bracketed by events for 20 further calls per route, and the
line also holds the mean device milliseconds per batch spent in each (torch's own kernels -- the draws, the concatenation --
are the remainder to the wall time)."""
import collections
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from amcontrast3d_amd import _lib, input_pipeline as ip  # noqa: E402
from amcontrast3d_amd.augment import ScanNetTrainAugment  # noqa: E402

STAGES = len(sys.argv) > 1 and sys.argv[1] == "stages"
VOXEL, REPS, CALLS = 0.02, 7, 50
SHAPES = ((2, 64000), (8, 32000))
SIDE = 280  # 2 * 280^2 = 156800 points per room
dev = torch.device("cuda:0")


def make_room(seed):
    """a raw ScanNet-like room: a 6.2 m floor with a relief and a second level, sampled on a 2.2 cm lattice twice with 3 mm
    jitter (a 2 cm voxel holds one to a few points); colours in [-1, 1], labels 0..19 with some -100"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij"), -1).reshape(-1, 2) * 0.022
    z = 0.4 * np.sin(ij[:, 0] + seed) * np.cos(0.7 * ij[:, 1]) + rng.choice([0.0, 0.8], len(ij))
    base = np.concatenate([ij, z[:, None]], 1) + np.array([-3.0, 1.0, 0.2])
    coord = np.concatenate([base + rng.uniform(-0.003, 0.003, base.shape) for _ in range(2)], 0).astype(np.float32)
    feat = rng.uniform(-1, 1, coord.shape).astype(np.float32)
    label = rng.integers(0, 20, len(coord)).astype(np.int64)
    label[rng.random(len(label)) < 0.03] = -100
    return tuple(torch.from_numpy(a).to(dev) for a in (coord, feat, label))


aug = ScanNetTrainAugment(color_drop=0.2, gravity_dim=2, rotate_dim=2, scale=[0.8, 1.2], mirror=[0.2, -1, -1], angle=1,
                          color_mean=ip.SCANNET_COLOR_MEAN, color_std=ip.SCANNET_COLOR_STD)
gen = torch.Generator(device=dev).manual_seed(0)
all_rooms = [make_room(200 + b) for b in range(max(b for b, _ in SHAPES))]
ENTRY_POINTS = [n for n in _lib.SIGNATURES if n.startswith(("amc3d_scannet_", "amc3d_voxel", "amc3d_crop_nearest"))
                and not n.endswith("_bytes")]


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def stage_times(routes, calls=20):
    """mean device ms per batch inside every C entry point, per route (events around each call)"""
    lib = _lib.load()
    real = {n: getattr(lib, n) for n in ENTRY_POINTS}
    log = []

    def bracket(name, fn):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a)
            e1.record()
            log.append((name, e0, e1))
            return r
        return call
    out = {}
    try:
        for n, fn in real.items():
            setattr(lib, n, bracket(n, fn))
        for k, fn in routes.items():
            del log[:]
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms = collections.defaultdict(float)
            for name, e0, e1 in log:
                ms[name.replace("amc3d_", "")] += e0.elapsed_time(e1) / calls
            out[k] = {name: round(v, 3) for name, v in ms.items()}
    finally:
        for n, fn in real.items():
            setattr(lib, n, fn)
    return out


def measure(B, voxel_max):
    rooms = all_rooms[:B]
    feed = ip.ScanNetTrainFeed(rooms, aug, batch_size=B, loop=CALLS, voxel_size=VOXEL, voxel_max=voxel_max, generator=gen)
    running = [iter(feed)]

    def from_feed():
        try:
            return next(running[0])
        except StopIteration:  # the next epoch: its permutation and room-level draws
            running[0] = iter(feed)
            return next(running[0])
    routes = {"per_room": lambda: ip.scannet_train_batch(rooms, aug, VOXEL, voxel_max, generator=gen),
              "joint": lambda: ip.scannet_train_rooms(rooms, aug, VOXEL, voxel_max, generator=gen),
              "feed": from_feed}
    for fn in routes.values():
        for _ in range(2):
            out = fn()
        assert out["pos"].shape == (B, voxel_max, 3)
    torch.cuda.synchronize()
    windows = {k: [] for k in routes}
    for _ in range(REPS):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / CALLS * 1e3)
    res = {"rooms": B, "voxel_max": voxel_max}
    res.update({k: stats(v) for k, v in windows.items()})
    res["joint_over_per_room"] = round(res["joint"]["median_ms"] / res["per_room"]["median_ms"], 3)
    res["feed_minus_joint_ms"] = round(res["feed"]["median_ms"] - res["joint"]["median_ms"], 3)
    if STAGES:
        res["stage_ms"] = stage_times(routes)
    return res


line = {"metric": "ScanNet training input, wall ms per batch of raw rooms (156800 points each, voxel 0.02 m, device generator)",
        "raw_points_per_room": 2 * SIDE * SIDE, "windows": REPS, "calls_per_window": CALLS,
        "shapes": [measure(B, vm) for B, vm in SHAPES]}
line["value"], line["unit"] = line["shapes"][0]["joint"]["median_ms"], "ms/batch"
print(json.dumps(line))
