"""Records tests/golden/scannet_eval.npz by RUNNING THE REFERENCE on the CPU (needs the reference tree; not run by the tests):

    python tests/tools/gen_golden_scannet_eval.py

ScanNet validation and whole-room testing as the reference does them, on small synthetic raw rooms written as .pth files:

  test route   `load_data` of examples/segmentation/main_AA.py (taken out of the file's syntax tree at run time: the file itself
               imports packages that are absent here), then per sub-cloud the steps of the cloud loop (main_AA.py:584-610) with
               the reference's own build_transforms_from_cfg('test', [PointsToTensor, NumpyChromaticNormalize]) and
               get_features_by_keys('pos,x,heights').
  val route    the reference's own ScanNet(split='val', presample=True, voxel_max=None) with build_transforms_from_cfg('val',
               [NumpyChromaticNormalize]); the randint draw of voxelize is logged.
  schedule     the reference's MultiStepLRScheduler, epochs 0..100, decay_epochs [70, 90], rate 0.1, with and without warm-up.

Two rooms: `a` (ordinary colours: the val route divides by 255) and `b` (dark: every colour <= 1 after (f + 1) * 127.5, so the
val route does not).  Per room `rows/<i>` holds, for sub-cloud i, the rows named in meta["rows"]: the transformed pos / x /
heights next to the channels of the assembled input they must equal (adjacent duplicates cost nothing once compressed)."""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
OUT = os.path.join(ROOT, "tests", "golden", "scannet_eval.npz")

import gen_golden_scannet as base  # noqa: E402  (loads the reference through oracle.refshim; make_room)

from openpoints.dataset.data_util import fnv_hash_vec, get_features_by_keys, voxelize  # noqa: E402  (reference)
from openpoints.dataset.scannetv2.scannet import ScanNet  # noqa: E402  (reference)
from openpoints.scheduler.multistep_lr import MultiStepLRScheduler  # noqa: E402  (reference)
from openpoints.transforms import build_transforms_from_cfg  # noqa: E402  (reference)
from openpoints.utils import EasyConfig  # noqa: E402

VOXEL = base.VOXEL
KWARGS = {"gravity_dim": 2, "color_mean": base.KWARGS["color_mean"], "color_std": base.KWARGS["color_std"]}
# the rows of rows/<i>: a recorded tensor's column, then the channel of the assembled (7, n) input that holds it
ROWS = ["pos0", "in0", "pos1", "in1", "pos2", "in2", "heights", "in6", "x0", "in3", "x1", "in4", "x2", "in5"]


def reference_load_data():
    """`load_data` compiled from the reference's main_AA.py syntax tree, with the reference's own voxelize in scope"""
    path = os.path.join(os.path.dirname(os.path.dirname(sys.modules["openpoints"].__file__)), "examples", "segmentation", "main_AA.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "load_data"]
    assert len(fn) == 1
    ns = {"np": np, "torch": torch, "voxelize": voxelize}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["load_data"]


def test_route(tag, path, load_data):
    cfg = EasyConfig()
    cfg.update({"dataset": {"common": {"NAME": "ScanNet", "voxel_size": VOXEL}, "test": {"split": "val"}},
                "feature_keys": "pos,x,heights"})
    tcfg = EasyConfig()
    tcfg.update({"test": ["PointsToTensor", "NumpyChromaticNormalize"], "kwargs": KWARGS})
    pipe = build_transforms_from_cfg("test", tcfg)
    np.random.seed(7)
    coord, feat, label, parts, voxel_idx, _, _ = load_data(path, cfg)
    # the tables load_data keeps to itself: the same function on the same input (deterministic)
    idx_sort, voxel_idx2, count = voxelize(coord, VOXEL, mode=1)
    assert np.array_equal(voxel_idx, voxel_idx2)
    start = np.cumsum(np.insert(count, 0, 0)[0:-1])
    P, nvox = int(count.max()), len(count)
    assert len(parts) == P
    voxel_of = np.empty(len(coord), np.int64)
    voxel_of[idx_sort] = voxel_idx
    out = {"shifted": coord, "test_feat": feat, "idx_sort": idx_sort.astype(np.int64), "voxel_idx": voxel_idx.astype(np.int64),
           "count": count.astype(np.int64), "parts": np.stack(parts).astype(np.int64)}
    for i, part in enumerate(parts):
        perm = voxel_of[part]  # the shuffle of part i, as a permutation of the voxel ids
        assert np.array_equal(np.sort(perm), np.arange(nvox)) and np.array_equal(idx_sort[start[perm] + i % count[perm]], part)
        # main_AA.py:584-610
        coord_part = coord[part]
        coord_part -= coord_part.min(0)
        data = pipe({"pos": coord_part, "x": feat[part]})
        data["heights"] = torch.from_numpy(coord_part[:, 2:3].astype(np.float32)).unsqueeze(0)
        data["x"] = data["x"].unsqueeze(0)
        data["pos"] = data["pos"].unsqueeze(0)
        pos, x, heights = data["pos"][0].numpy().copy(), data["x"][0].numpy().copy(), data["heights"][0].numpy().copy()
        inp = get_features_by_keys(data, cfg.feature_keys)[0].numpy()
        assert inp.shape == (7, nvox) and pos.dtype == x.dtype == heights.dtype == inp.dtype == np.float32
        named = {"pos0": pos[:, 0], "pos1": pos[:, 1], "pos2": pos[:, 2], "heights": heights[:, 0], "x0": x[:, 0], "x1": x[:, 1],
                 "x2": x[:, 2], **{f"in{c}": inp[c] for c in range(7)}}
        out[f"rows/{i}"] = np.stack([named[k] for k in ROWS])
    # what makes the fixture bite: sparse and dense voxels, and points of one voxel with different numbers of votes
    assert (count == 1).any() and (count == 2).any() and (count >= 3).any() and (P % count != 0).any()
    print(tag, "test route: points", len(coord), "voxels", nvox, "parts", P, "count histogram", np.bincount(count).tolist())
    return out


def val_route(tag, tmp, path):
    tcfg = EasyConfig()
    tcfg.update({"val": ["NumpyChromaticNormalize"], "kwargs": KWARGS})
    transform = build_transforms_from_cfg("val", tcfg)
    log = []
    orig = np.random.randint

    def randint(*a, **k):
        v = orig(*a, **k)
        log.append(np.array(v))
        return v
    np.random.randint = randint
    try:
        ds = ScanNet(data_root=tmp, split="val", voxel_size=VOXEL, voxel_max=None, transform=transform, presample=True)
    finally:
        np.random.randint = orig
    assert len(log) == 1 and len(ds.data_list) == 1 and ds.data_list[0] == path
    rnd = log[0].astype(np.int64)
    item = ds[0]
    coord, feat, label = torch.load(path)
    shifted = coord - coord.min(0)
    key = fnv_hash_vec(np.floor(shifted / np.array(VOXEL)))
    idx_sort = np.argsort(key)
    _, count = np.unique(key[idx_sort], return_counts=True)
    idx_unique = idx_sort[np.cumsum(np.insert(count, 0, 0)[0:-1]) + rnd % count]
    sel = shifted[idx_unique]
    assert np.array_equal((sel - sel.min(0)).astype(np.float32), item["pos"].numpy())  # the picks are the reference's
    batch = {k: item[k].unsqueeze(0) for k in ("pos", "x", "heights")}
    inp = get_features_by_keys(batch, "pos,x,heights")[0].numpy()
    x = item["x"].numpy()
    raw_max = float(((feat[idx_unique] + 1) * 127.5).max())
    print(tag, "val route: voxels", len(idx_unique), "colour max before the normalisation", raw_max)
    return {"val/rnd": rnd, "val/idx_unique": idx_unique.astype(np.int64), "val/pos": item["pos"].numpy(), "val/x": x,
            "val/heights": item["heights"].numpy(), "val/y": item["y"].numpy().astype(np.int64), "val/input": inp}, raw_max


def schedules():
    out = {}
    for tag, warm in (("plain", 0), ("warmup", 5)):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=0.001)
        s = MultiStepLRScheduler(opt, decay_t=[70, 90], decay_rate=0.1, warmup_t=warm, warmup_lr_init=1.0e-6)
        out[f"sched/{tag}/initial"] = np.float64(opt.param_groups[0]["lr"])
        out[f"sched/{tag}/lr"] = np.array([s.get_epoch_values(t)[0] for t in range(101)], dtype=np.float64)
    return out


def main():
    _load = torch.load
    torch.load = lambda *a, **k: _load(*a, **dict(k, weights_only=False))  # the .pth rooms hold numpy arrays
    load_data = reference_load_data()
    out = {}
    rooms = {"a": base.make_room(910, 1500, 2, 31), "b": base.make_room(911, 450, 2, 32)}
    c, f, l = rooms["b"]
    rooms["b"] = (c, (-1 + (f + 1) * np.float32(0.5 / 127.5)).astype(np.float32), l)  # dark: (f + 1) * 127.5 <= 1
    for tag, (coord, feat, label) in rooms.items():
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "val"))
            path = os.path.join(tmp, "val", f"room_{tag}.pth")
            torch.save((coord, feat, label), path)
            o = {"coord": coord, "feat": feat, "label": label}
            o.update(test_route(tag, path, load_data))
            assert np.array_equal(o.pop("shifted"), coord - coord.min(0))
            assert np.array_equal(o.pop("test_feat"), np.clip((feat + 1) / 2., 0, 1).astype(np.float32))
            v, raw_max = val_route(tag, tmp, path)
            assert (raw_max > 1) == (tag == "a")
            o.update(v)
        out.update({f"{tag}/{k}": v for k, v in o.items()})
    out.update(schedules())
    meta = {"numpy": np.__version__, "voxel_size": VOXEL, "kwargs": KWARGS, "rows": ROWS, "feature_keys": "pos,x,heights",
            "sched": {"lr": 0.001, "decay_epochs": [70, 90], "decay_rate": 0.1, "warmup_epochs": 5, "warmup_lr": 1.0e-6}}
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
