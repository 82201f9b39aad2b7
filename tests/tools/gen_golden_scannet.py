"""Records tests/golden/scannet_input.npz by RUNNING THE REFERENCE on the CPU (needs the reference tree; not run by the tests):

    python tests/tools/gen_golden_scannet.py

The reference's own ScanNet.__getitem__ (dataset/scannetv2/scannet.py:140-176) with its own training transforms
(cfgs/scannet/default.yaml datatransforms: RandomRotateZ, RandomScale, ChromaticAutoContrast, RandomDropFeature,
NumpyChromaticNormalize, built by build_transforms_from_cfg) runs on small synthetic raw rooms written as .pth files.  Every
random number is logged by wrapping np.random.uniform / rand / randint / choice / permutation.  Stored per case: the inputs,
R (scipy's expm, recomputed by the class's own M), the draws, the whole-room transformed pos (float64) and x (float32), the
voxel keys, idx_unique (the reference's unstable argsort, recomputed on the same input), the crop distances and crop_idx,
and the final pos / x / y / heights.  Two cases:
  a: contrast taken, mirror taken, drop not taken, N >= voxel_max (a crop happens);
  b: contrast not taken, drop taken (max <= 1: no /255), N < voxel_max with variable=False (padded by repetition)."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "scannet_input.npz")

from oracle import refshim  # noqa: E402

refshim.load_reference()

from openpoints.dataset.data_util import fnv_hash_vec  # noqa: E402  (reference)
from openpoints.dataset.scannetv2.scannet import ScanNet  # noqa: E402  (reference)
from openpoints.transforms import build_transforms_from_cfg  # noqa: E402  (reference)
from openpoints.transforms.point_transform_cpu import RandomRotateZ  # noqa: E402  (reference)
from openpoints.utils import EasyConfig  # noqa: E402

from amcontrast3d_amd import synthetic  # noqa: E402  (plain numpy helper)

KWARGS = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
          "color_mean": [0.46259782, 0.46253258, 0.46253258], "color_std": [0.693565, 0.6852543, 0.68061745]}
TRAIN = ["RandomRotateZ", "RandomScale", "ChromaticAutoContrast", "RandomDropFeature", "NumpyChromaticNormalize"]
VOXEL = 0.02


def make_room(first_id, n_base, copies, seed):
    """a raw room: jittered copies of a synthetic scene, several points per 2 cm voxel; colours in [-1, 1], labels with -100"""
    room = synthetic.make_batch(1, n_base, first_id=first_id, voxel_size=VOXEL)
    rng = np.random.default_rng(seed)
    base = room["pos"][0].astype(np.float32) + np.float32([1.5, -2.0, 0.1])  # not at the origin: the shifts matter
    coord = np.concatenate([base + rng.uniform(-0.012, 0.012, base.shape).astype(np.float32) for _ in range(copies)], 0)
    feat = np.concatenate([room["x"][0, :3].T] * copies, 0).astype(np.float32) * 2 - 1
    label = np.concatenate([room["y"][0]] * copies, 0).astype(np.int64) % 20
    label[rng.random(len(label)) < 0.05] = -100
    perm = rng.permutation(len(coord))
    return coord[perm].astype(np.float32), feat[perm].astype(np.float32), label[perm]


def pattern(seed, want):
    """the transform draws a seed gives (same calls in the same order as the classes): contrast / mirror / drop taken?"""
    np.random.seed(seed)
    np.random.uniform(-np.pi, np.pi)
    np.random.uniform(0.8, 1.2, 1)
    mirror = np.random.rand(3)[0] <= 0.2
    contrast = np.random.rand() < 0.2
    if contrast:
        np.random.rand()
    drop = np.random.rand() < 0.2
    return (contrast, mirror, drop) == want


def run_case(tag, room, voxel_max, want, tmp):
    coord, feat, label = room
    seed = next(s for s in range(10000) if pattern(s, want))
    path = os.path.join(tmp, "train", f"room_{tag}.pth")
    torch.save((coord, feat, label), path)
    tcfg = EasyConfig()
    tcfg.update({"train": TRAIN, "kwargs": KWARGS})
    transform = build_transforms_from_cfg("train", tcfg)
    ds = ScanNet(data_root=tmp, split="train", voxel_size=VOXEL, voxel_max=voxel_max, transform=transform, variable=False)
    ds.data_list = [path]
    # what the transforms hand to crop_pc (the whole transformed room), recorded on the way
    seen = {}
    inner = transform.__call__

    class Spy:
        def __call__(self, data):
            data = inner(data)
            seen["pos"], seen["x"] = data["pos"].copy(), data["x"].copy()
            return data
    ds.transform = Spy()
    log = []
    names = ("uniform", "rand", "randint", "choice", "permutation")
    orig = {n: getattr(np.random, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            v = orig[n](*a, **k)
            log.append((n, np.array(v)))
            return v
        return f
    for n in names:
        setattr(np.random, n, wrap(n))
    try:
        np.random.seed(seed)
        data = ds[0]
    finally:
        for n in names:
            setattr(np.random, n, orig[n])
    kinds = [k for k, _ in log]
    i = 0
    out = {}
    assert kinds[i] == "uniform"; angle = float(log[i][1]); i += 1
    assert kinds[i] == "uniform"; scale = log[i][1].astype(np.float64); i += 1
    assert kinds[i] == "rand"; mirror_u = log[i][1]; i += 1
    assert kinds[i] == "rand"; contrast_u = float(log[i][1]); i += 1
    blend = np.nan
    if contrast_u < 0.2:
        blend = float(log[i][1]); i += 1
    assert kinds[i] == "rand"; drop_u = float(log[i][1]); i += 1
    assert kinds[i] == "randint"; rnd = log[i][1].astype(np.int64); i += 1
    init_idx, pad = np.int64(-1), np.zeros(0, np.int64)
    if kinds[i] == "randint":
        init_idx = np.int64(log[i][1]); i += 1
    else:
        assert kinds[i] == "choice"; pad = log[i][1].astype(np.int64); i += 1
    assert kinds[i] == "permutation"; perm = log[i][1].astype(np.int64); i += 1
    assert i == len(log), kinds
    axis = np.zeros(3); axis[2] = 1
    R = RandomRotateZ.M(axis, angle)
    # the intermediates of crop_pc, recomputed with the reference's own functions on the same input (deterministic)
    coord_s = seen["pos"] - seen["pos"].min(0)
    key = fnv_hash_vec(np.floor(coord_s / np.array(VOXEL)))
    idx_sort = np.argsort(key)
    _, count = np.unique(key[idx_sort], return_counts=True)
    idx_unique = idx_sort[np.cumsum(np.insert(count, 0, 0)[0:-1]) + rnd % count]
    cv = coord_s[idx_unique]
    N = len(idx_unique)
    d2, crop_idx = np.zeros(0), np.zeros(0, np.int64)
    if N >= voxel_max:
        d2 = np.sum(np.square(cv - cv[init_idx]), 1)
        crop_idx = np.argsort(d2)[:voxel_max]
        final = cv[crop_idx[perm]]
    else:
        final = cv[np.hstack([np.arange(N), pad])[perm]]
    final = (final - final.min(0)).astype(np.float32)
    assert np.array_equal(final, data["pos"].numpy())
    out.update({"coord": coord, "feat": feat, "label": label, "voxel_max": np.int64(voxel_max), "R": R,
                "angle": np.float64(angle), "scale": scale, "mirror_u": mirror_u, "contrast_u": np.float64(contrast_u),
                "blend": np.float64(blend), "drop_u": np.float64(drop_u), "rnd": rnd, "init_idx": init_idx, "pad": pad,
                "perm": perm, "t_pos": seen["pos"], "t_x": seen["x"], "key": key, "count": count.astype(np.int64),
                "idx_unique": idx_unique.astype(np.int64), "d2": d2, "crop_idx": crop_idx.astype(np.int64),
                "pos": data["pos"].numpy(), "x": data["x"].numpy(), "y": data["y"].numpy().astype(np.int64),
                "heights": data["heights"].numpy()})
    assert out["t_pos"].dtype == np.float64 and out["t_x"].dtype == np.float32
    print(tag, "seed", seed, "raw", len(coord), "voxels", N, "voxel_max", voxel_max, "contrast", contrast_u < 0.2,
          "mirror", bool(mirror_u[0] <= 0.2), "drop", drop_u < 0.2, "x max", float(np.nanmax(seen["x"])))
    return {f"{tag}/{k}": v for k, v in out.items()}


def main():
    _load = torch.load
    torch.load = lambda *a, **k: _load(*a, **dict(k, weights_only=False))  # the .pth rooms hold numpy arrays
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "train"))
        out.update(run_case("a", make_room(900, 1500, 3, 21), 900, (True, True, False), tmp))
        out.update(run_case("b", make_room(901, 1500, 3, 22), 3000, (False, False, True), tmp))
    import numpy.__config__  # noqa: F401
    try:
        import threadpoolctl
        blas = [d.get("version") for d in threadpoolctl.threadpool_info() if d.get("internal_api") == "openblas"]
    except Exception:
        blas = []
    cfg = np.show_config(mode="dicts") if "mode" in np.show_config.__code__.co_varnames else {}
    blas_cfg = cfg.get("Build Dependencies", {}).get("blas", {}) if isinstance(cfg, dict) else {}
    meta = {"numpy": np.__version__, "openblas": blas or blas_cfg.get("version"), "voxel_size": VOXEL, "kwargs": KWARGS,
            "note": "np.dot(pos_f32, R_f64) through OpenBLAS dgemm: fma(p2, R[2,j], fma(p1, R[1,j], p0 * R[0,j]))"}
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes", meta["openblas"])


if __name__ == "__main__":
    main()
