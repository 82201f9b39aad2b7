"""Records tests/golden/s3dis_input.npz by RUNNING THE REFERENCE on the CPU (needs the reference tree; not run by the tests):

    python tests/tools/gen_golden_s3dis_input.py

The reference's own S3DIS.__getitem__ with presample=False (dataset/s3dis/s3dis.py:122-144) and its own training transforms
(cfgs/s3dis/default.yaml datatransforms.train with the config's kwargs, built by build_transforms_from_cfg) runs on two small
synthetic raw rooms written as float64 raw/Area_1_*.npy.  Every random number is logged by wrapping the numpy and torch
generator functions the item calls.  Stored per case: the raw room, the draws, the voxel keys and counts, idx_unique and the crop
(the reference's unstable argsort, recomputed with its own functions on the same input), the cropped cloud before the
transforms and the final pos / x / y / heights.  Two cases:
  a: N >= voxel_max (a crop happens), auto-contrast taken, colours kept;
  b: N < voxel_max with variable=False (padded by repetition), no auto-contrast, colour drop taken."""
import collections
import collections.abc
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "s3dis_input.npz")

from oracle import refshim  # noqa: E402

refshim.load_reference()
if not hasattr(collections, "Iterable"):
    collections.Iterable = collections.abc.Iterable  # removed from `collections` in Python 3.10; PointCloudRotation reads it

from openpoints.dataset.data_util import fnv_hash_vec  # noqa: E402  (reference)
from openpoints.dataset.s3dis.s3dis import S3DIS  # noqa: E402  (reference)
from openpoints.transforms import build_transforms_from_cfg  # noqa: E402  (reference)
from openpoints.utils import EasyConfig  # noqa: E402

from amcontrast3d_amd import synthetic  # noqa: E402  (plain numpy helper)

KWARGS = {"color_drop": 0.2, "gravity_dim": 2, "scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02}
TRAIN = ["ChromaticAutoContrast", "PointsToTensor", "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation",
         "PointCloudJitter", "ChromaticDropGPU", "ChromaticNormalize"]  # cfgs/s3dis/default.yaml:33-43
VOXEL = 0.04
NP_NAMES = ("rand", "uniform", "randint", "choice", "permutation", "shuffle")


def make_room(first_id, n_base, copies, seed):
    """a raw room as np.load gives an Area_*.npy: float64 (n,7) = xyz, rgb 0..255, label; jittered copies of a synthetic
    scene, several points per 4 cm voxel, away from the origin"""
    room = synthetic.make_batch(1, n_base, first_id=first_id, voxel_size=VOXEL)
    rng = np.random.default_rng(seed)
    base = room["pos"][0].astype(np.float64) + np.array([12.5, -7.25, 0.3])  # not at the origin: the shifts matter
    xyz = np.concatenate([base + rng.uniform(-0.02, 0.02, base.shape) for _ in range(copies)], 0)
    rgb = np.concatenate([np.round(room["x"][0, :3].T * 255.0)] * copies, 0).astype(np.float64)
    label = np.concatenate([room["y"][0]] * copies, 0).astype(np.float64) % 13
    perm = rng.permutation(len(xyz))
    return np.ascontiguousarray(np.concatenate([xyz, rgb, label[:, None]], 1)[perm])


def run_item(ds, seed):
    """ds[0] from one seed, with every draw logged in order -> (item, log)"""
    log = []
    orig_np = {n: getattr(np.random, n) for n in NP_NAMES}
    orig_t = (torch.rand, torch.randn_like)

    def wrap(n):
        def f(*a, **k):
            v = orig_np[n](*a, **k)
            log.append(("np." + n, None if v is None else np.array(v)))
            return v
        return f

    def t_wrap(name, fn):
        def f(*a, **k):
            v = fn(*a, **k)
            log.append((name, v.clone().numpy()))
            return v
        return f
    for n in NP_NAMES:
        setattr(np.random, n, wrap(n))
    torch.rand, torch.randn_like = t_wrap("torch.rand", orig_t[0]), t_wrap("torch.randn_like", orig_t[1])
    try:
        np.random.seed(seed)
        torch.manual_seed(seed)
        item = ds[0]
    finally:
        for n in NP_NAMES:
            setattr(np.random, n, orig_np[n])
        torch.rand, torch.randn_like = orig_t
    return item, log


def parse(log, N, voxel_max):
    """the draws by name, in the order S3DIS.__getitem__ makes them: crop_pc's, then the transform chain's"""
    kinds = [k for k, _ in log]
    i = 0
    d = {}
    assert kinds[i] == "np.randint"; d["rnd"] = log[i][1].astype(np.int64); i += 1
    d["init_idx"], d["pad"] = np.int64(-1), np.zeros(0, np.int64)
    if N >= voxel_max:
        assert kinds[i] == "np.randint"; d["init_idx"] = np.int64(log[i][1]); i += 1
    else:
        assert kinds[i] == "np.choice"; d["pad"] = log[i][1].astype(np.int64); i += 1
    assert kinds[i] == "np.permutation"; d["perm"] = log[i][1].astype(np.int64); i += 1
    assert kinds[i] == "np.rand"; d["contrast_u"] = np.float64(log[i][1]); i += 1
    d["blend"] = np.float64(0.0)
    if d["contrast_u"] < 0.2:
        assert kinds[i] == "np.rand"; d["blend"] = np.float64(log[i][1]); i += 1
    assert kinds[i] == "torch.rand" and log[i][1].shape == (3,); d["scale_u"] = log[i][1]; i += 1
    assert kinds[i:i + 3] == ["np.uniform"] * 3
    d["theta"] = np.array([log[i][1], log[i + 1][1], log[i + 2][1]], dtype=np.float64); i += 3
    assert kinds[i] == "np.shuffle"; i += 1  # the order of the three rotations: two are the identity (angle [0, 0, 1])
    assert d["theta"][0] == 0 and d["theta"][1] == 0
    assert kinds[i] == "torch.randn_like"; d["noise"] = log[i][1]; i += 1
    assert kinds[i] == "torch.rand" and log[i][1].shape == (1,); d["drop_u"] = np.float64(log[i][1][0]); i += 1
    assert i == len(log), kinds
    return d


def run_case(tag, cdata, voxel_max, want, tmp):
    raw = os.path.join(tmp, tag, "raw")
    os.makedirs(raw)
    np.save(os.path.join(raw, f"Area_1_{tag}.npy"), cdata)
    tcfg = EasyConfig()
    tcfg.update({"train": TRAIN, "kwargs": KWARGS})
    ds = S3DIS(data_root=os.path.join(tmp, tag), test_area=5, voxel_size=VOXEL, voxel_max=voxel_max, split="train",
               transform=build_transforms_from_cfg("train", tcfg), loop=1, presample=False, variable=False, shuffle=True)
    assert len(ds) == 1
    # the voxel count, from the reference's own hash on the same input
    c = cdata.astype(np.float32)
    c[:, :3] -= np.min(c[:, :3], 0)
    coord = c[:, :3] - c[:, :3].min(0)
    key = fnv_hash_vec(np.floor(coord / np.array(VOXEL)))
    idx_sort = np.argsort(key)
    _, count = np.unique(key[idx_sort], return_counts=True)
    N = len(count)
    for seed in range(10000):
        item, log = run_item(ds, seed)
        d = parse(log, N, voxel_max)
        if (d["contrast_u"] < 0.2, d["drop_u"] < 0.2) == want:
            break
    else:
        raise RuntimeError("no seed gives the wanted branches")
    # the intermediates of crop_pc, recomputed with the reference's own functions on the same input (deterministic)
    idx_unique = idx_sort[np.cumsum(np.insert(count, 0, 0)[0:-1]) + d["rnd"] % count]
    cv = coord[idx_unique]
    d2, crop_idx = np.zeros(0, np.float32), np.zeros(0, np.int64)
    if N >= voxel_max:
        d2 = np.sum(np.square(cv - cv[d["init_idx"]]), 1)
        crop_idx = np.argsort(d2)[:voxel_max]
        idx = crop_idx[d["perm"]]
    else:
        idx = np.hstack([np.arange(N), d["pad"]])[d["perm"]]
    pos0 = cv[idx]
    pos0 = (pos0 - pos0.min(0)).astype(np.float32)
    heights = item["heights"].numpy()
    assert np.array_equal(pos0[:, 2:3], heights)  # s3dis.py:142-143: the cropped cloud's gravity column
    assert np.array_equal(c[idx_unique][idx][:, 6].astype(np.int64), item["y"].numpy())
    assert d2.dtype == np.float32 and item["pos"].dtype == torch.float32 and item["x"].dtype == torch.float32
    out = {"cdata": cdata, "voxel_max": np.int64(voxel_max), "key": key, "count": count.astype(np.int32),
           "idx_unique": idx_unique.astype(np.int32), "d2": d2, "crop_idx": crop_idx.astype(np.int32), "pos0": pos0,
           "pos": item["pos"].numpy(), "x": item["x"].numpy(), "y": item["y"].numpy().astype(np.int64), "heights": heights}
    out.update({k: (v.astype(np.int32) if k in ("rnd", "pad", "perm") else v) for k, v in d.items()})
    print(tag, "seed", seed, "raw", len(cdata), "voxels", N, "count.max", int(count.max()), "voxel_max", voxel_max, "contrast",
          bool(d["contrast_u"] < 0.2), "drop", bool(d["drop_u"] < 0.2))
    return {f"{tag}/{k}": v for k, v in out.items()}


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        out.update(run_case("a", make_room(910, 1500, 3, 31), 900, (True, False), tmp))
        out.update(run_case("b", make_room(911, 1500, 3, 32), 2000, (False, True), tmp))
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__, "voxel_size": VOXEL, "kwargs": KWARGS,
                                       "train": TRAIN}))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
