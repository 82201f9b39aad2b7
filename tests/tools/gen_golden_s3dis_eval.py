"""Records tests/golden/s3dis_eval.npz by RUNNING THE REFERENCE on the CPU (needs the reference tree; not run by the tests):

    python tests/tools/gen_golden_s3dis_eval.py

S3DIS validation and whole-room testing as the reference does them, on small synthetic raw rooms written as Area_5_*.npy:

  test route   `load_data` of examples/segmentation/main.py (taken out of the file's syntax tree at run time: the file itself
               imports packages that are absent here), in both test modes, then per sub-cloud the steps of the cloud loop
               (main.py:562-587) with the reference's own build_transforms_from_cfg('val', [PointsToTensor, PointCloudXYZAlign,
               ChromaticNormalize]) -- cfgs/s3dis/default.yaml has no `test` list, so test() takes `val` -- and
               get_features_by_keys('x,heights').
  val route    the reference's own S3DIS(split='val', presample=True, voxel_max=None) on a temporary data root with the same
               transforms; the randint draw of voxelize is logged.

Two rooms: `a` is float64 with ordinary colours (the val route divides by 255), `b` is float32 and dark (every raw colour
<= 1, so the val route does not).  The rooms are stored compactly and exactly: a's coordinates as int32 multiples of 2**-26
(29 significant bits: not float32 numbers, so float64 arithmetic before the cast matters), the colours as uint8 k with
colour = k (a) or float32(k) / float32(255) (b); tests/s3dis_eval_ref.py:fixture_cdata rebuilds the (n,7) arrays.

Per room and route, `full/<i>` holds every row of sub-cloud i and `rows/<i>` the points meta["pick"] selects (the same
positions in every sub-cloud), both in the layout meta["rows"]: the transformed pos / x / heights next to the channels of the
assembled (4, n) input they must equal (adjacent duplicates cost nothing once compressed).  `centre` is torch.mean's own
centre per sub-cloud -- its last bit depends on this host's vector width and thread count -- and meta["centre_ulp"] the
largest distance in ulp between it and the exactly rounded mean (math.fsum) over everything recorded."""
import ast
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "s3dis_eval.npz")

from oracle import refshim  # noqa: E402

refshim.load_reference()

from openpoints.dataset.data_util import get_features_by_keys, voxelize  # noqa: E402  (reference)
from openpoints.dataset.s3dis.s3dis import S3DIS  # noqa: E402  (reference)
from openpoints.transforms import build_transforms_from_cfg  # noqa: E402  (reference)
from openpoints.utils import EasyConfig  # noqa: E402

import s3dis_eval_ref as ours  # noqa: E402  (make_raw_room / fixture_cdata only: the rooms, not the arithmetic)

VOXEL = ours.VOXEL
GRAVITY = 2
TRANSFORMS = ["PointsToTensor", "PointCloudXYZAlign", "ChromaticNormalize"]
# a recorded tensor's column, then the channel of the assembled (4, n) input that holds it
ROWS = ["pos0", "pos1", "pos2", "heights", "in3", "x0", "in0", "x1", "in1", "x2", "in2"]
FULL = {"a": [1], "b": [0]}  # the test-route sub-clouds recorded in full
N_PICK = 48


def reference_load_data():
    """`load_data` compiled from the reference's main.py syntax tree, with the reference's own voxelize in scope"""
    path = os.path.join(os.path.dirname(os.path.dirname(sys.modules["openpoints"].__file__)), "examples", "segmentation", "main.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "load_data"]
    assert len(fn) == 1
    ns = {"np": np, "torch": torch, "voxelize": voxelize}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["load_data"]


def pipeline(split="val"):
    tcfg = EasyConfig()
    tcfg.update({"val": TRANSFORMS, "kwargs": {"gravity_dim": GRAVITY}})  # ChromaticNormalize: the class's default constants
    return build_transforms_from_cfg(split, tcfg)


def exact_centre(q):
    """fl32 of the exact mean of the float32 columns of q; also the relative distance of the exact mean to the nearest
    float32 rounding boundary"""
    n = len(q)
    out, ties = np.empty(3, np.float32), []
    for c in range(3):
        s = math.fsum(float(v) for v in q[:, c])  # exactly rounded float64 sum
        m = s / n
        out[c] = np.float32(m)
        lo, hi = np.nextafter(out[c], np.float32(-np.inf)), np.nextafter(out[c], np.float32(np.inf))
        edge = min(abs((float(lo) + float(out[c])) / 2 - m), abs((float(hi) + float(out[c])) / 2 - m))
        ties.append(edge / abs(m))
    return out, min(ties)


def ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


STATS = {"ulp": 0, "edge": np.inf}


def transformed(pipe, coord_part, feat_part, cfg):
    """main.py:563-587 on one sub-cloud; coord_part is already shifted (the caller's in-place -=, as the loop has it)"""
    data = pipe({"pos": coord_part, "x": feat_part})
    q32 = coord_part.astype(np.float32)
    data["heights"] = torch.from_numpy(coord_part[:, GRAVITY:GRAVITY + 1].astype(np.float32)).unsqueeze(0)
    data["x"] = data["x"].unsqueeze(0)
    data["pos"] = data["pos"].unsqueeze(0)
    pos, x, heights = data["pos"][0].numpy().copy(), data["x"][0].numpy().copy(), data["heights"][0].numpy().copy()
    inp = get_features_by_keys(data, cfg.feature_keys)[0].numpy()
    return record(pos, x, heights, inp, q32)


def record(pos, x, heights, inp, q32):
    n = len(pos)
    assert inp.shape == (4, n) and pos.dtype == x.dtype == heights.dtype == inp.dtype == np.float32
    centre = torch.mean(torch.from_numpy(q32.copy()), axis=0, keepdims=True)[0].numpy()  # the call PointCloudXYZAlign makes
    # it is the centre the transform used: pos (before the gravity column's shift) = q - centre
    for c in range(3):
        if c != GRAVITY:
            assert np.array_equal(pos[:, c], q32[:, c] - centre[c])
    exact, edge = exact_centre(q32)
    STATS["ulp"] = max(STATS["ulp"], ulp_distance(centre, exact))
    STATS["edge"] = min(STATS["edge"], edge)
    named = {"pos0": pos[:, 0], "pos1": pos[:, 1], "pos2": pos[:, 2], "heights": heights[:, 0], "x0": x[:, 0], "x1": x[:, 1],
             "x2": x[:, 2], **{f"in{c}": inp[c] for c in range(4)}}
    return np.stack([named[k] for k in ROWS]), centre


def test_route(tag, path, load_data):
    cfg = EasyConfig()
    cfg.update({"dataset": {"common": {"NAME": "S3DIS", "voxel_size": VOXEL}, "test": {"split": "val"}}, "feature_keys": "x,heights"})
    pipe = pipeline()
    np.random.seed(7)
    coord, feat, label, parts, voxel_idx, rev_part, rev_sort = load_data(path, cfg)
    assert rev_part is None and rev_sort is None
    # the tables load_data keeps to itself: the same function on the same input (deterministic)
    idx_sort, voxel_idx2, count = voxelize(coord, VOXEL, mode=1)
    assert np.array_equal(voxel_idx, voxel_idx2)
    start = np.cumsum(np.insert(count, 0, 0)[0:-1])
    P, nvox = int(count.max()), len(count)
    assert len(parts) == P
    voxel_of = np.empty(len(coord), np.int64)
    voxel_of[idx_sort] = voxel_idx
    pick = np.sort(np.random.default_rng(3).choice(nvox, N_PICK, replace=False))
    out = {"pick": pick.astype(np.int16), "shifted": coord, "test_feat": feat, "idx_sort": idx_sort.astype(np.int16), "voxel_idx": voxel_idx.astype(np.int16),
           "count": count.astype(np.int16), "parts": np.stack(parts).astype(np.int16), "centre": np.empty((P, 3), np.float32)}
    for i, part in enumerate(parts):
        perm = voxel_of[part]  # the shuffle of part i, as a permutation of the voxel ids
        assert np.array_equal(np.sort(perm), np.arange(nvox)) and np.array_equal(idx_sort[start[perm] + i % count[perm]], part)
        coord_part = coord[part]
        coord_part -= coord_part.min(0)
        rows, out["centre"][i] = transformed(pipe, coord_part, feat[part], cfg)
        out[f"rows/{i}"] = rows[:, pick]
        if i in FULL[tag]:
            out[f"full/{i}"] = rows
    print(tag, "test route: points", len(coord), coord.dtype, "voxels", nvox, "parts", P, "count histogram", np.bincount(count).tolist())

    # test_mode nearest_neighbor: the same tables (voxelize is deterministic), one sub-cloud of representatives
    cfg.test_mode = "nearest_neighbor"
    log = {}
    orig_randint, orig_perm = np.random.randint, np.random.permutation

    def randint(*a, **k):
        log["rnd"] = np.array(orig_randint(*a, **k))
        return log["rnd"]

    def permutation(*a, **k):
        log["perm"] = np.array(orig_perm(*a, **k))
        return log["perm"]
    np.random.seed(8)
    np.random.randint, np.random.permutation = randint, permutation
    try:
        coord2, feat2, _, parts2, voxel_idx3, rev_part, rev_sort = load_data(path, cfg)
    finally:
        np.random.randint, np.random.permutation = orig_randint, orig_perm
    assert np.array_equal(coord2, coord) and np.array_equal(voxel_idx3, voxel_idx) and len(parts2) == 1
    part = parts2[0]
    assert np.array_equal(part, idx_sort[start + log["rnd"] % count][log["perm"]])
    coord_part = coord[part]
    coord_part -= coord_part.min(0)
    rows, centre = transformed(pipe, coord_part, feat[part], cfg)
    # main.py:605 applied to the positions 0..nvox-1 of the sub-cloud: which of its rows every room point takes
    expand = np.arange(nvox)[rev_part][voxel_idx][rev_sort]
    assert np.array_equal(voxel_of[part[expand]], voxel_of)  # a point of the same voxel
    out.update({"nn/rnd": log["rnd"].astype(np.int16), "nn/perm": log["perm"].astype(np.int16), "nn/part": part.astype(np.int16),
                "nn/where": rev_part.astype(np.int16), "nn/expand": expand.astype(np.int16), "nn/rows": rows[:, pick],
                "nn/centre": centre})
    return out


def val_route(tag, cdata):
    log = []
    orig = np.random.randint

    def randint(*a, **k):
        v = orig(*a, **k)
        log.append(np.array(v))
        return v
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "raw"))
        np.save(os.path.join(tmp, "raw", f"Area_5_{tag}.npy"), cdata)
        np.random.randint = randint
        try:
            ds = S3DIS(data_root=tmp, test_area=5, voxel_size=VOXEL, voxel_max=None, split="val", transform=pipeline(), presample=True)
        finally:
            np.random.randint = orig
        assert len(log) == 1 and len(ds) == 1
        rnd = log[0].astype(np.int64)
        pre = ds.data[0].copy()
        item = ds[0]
    c32 = cdata.astype(np.float32)
    shifted = c32[:, :3] - np.min(c32[:, :3], 0)
    # the tables voxelize kept to itself (deterministic on the same input)
    idx_sort, _, count = voxelize(shifted, VOXEL, mode=1)
    idx_unique = idx_sort[np.cumsum(np.insert(count, 0, 0)[0:-1]) + rnd % count]
    assert np.array_equal(pre[:, :3], shifted[idx_unique]) and np.array_equal(pre[:, 3:6], c32[idx_unique, 3:6])
    batch = {k: item[k].unsqueeze(0) for k in ("pos", "x", "heights")}
    inp = get_features_by_keys(batch, "x,heights")[0].numpy()
    rows, centre = record(item["pos"].numpy(), item["x"].numpy(), item["heights"].numpy(), inp, shifted[idx_unique])
    raw_max = float(c32[idx_unique, 3:6].max())
    print(tag, "val route: voxels", len(idx_unique), "colour maximum before the normalisation", raw_max)
    return {"val/rnd": rnd.astype(np.int16), "val/idx_sort": idx_sort.astype(np.int16), "val/count": count.astype(np.int16),
            "val/idx_unique": idx_unique.astype(np.int16), "val/full": rows, "val/centre": centre,
            "val/y": item["y"].numpy().astype(np.int16)}, raw_max


def main():
    load_data = reference_load_data()
    out = {}
    for tag in ("a", "b"):
        stored = ours.make_raw_room(tag)
        cdata = ours.fixture_cdata(stored)
        assert cdata.dtype == (np.float64 if tag == "a" else np.float32) and cdata.shape[1] == 7
        o = dict(stored)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, f"Area_5_{tag}.npy")
            np.save(path, cdata)
            o.update(test_route(tag, path, load_data))
        shifted = o.pop("shifted")
        assert shifted.dtype == cdata.dtype and np.array_equal(shifted, cdata[:, :3] - cdata[:, :3].min(0))
        assert np.array_equal(o.pop("test_feat"), np.clip(cdata[:, 3:6] / 255., 0, 1).astype(np.float32))
        v, raw_max = val_route(tag, cdata)
        assert (raw_max > 1) == (tag == "a")
        o.update(v)
        out.update({f"{tag}/{k}": v for k, v in o.items()})
        print(tag, "so far: centre within", STATS["ulp"], "ulp, nearest rounding boundary (relative)", STATS["edge"])
    meta = {"numpy": np.__version__, "torch": torch.__version__, "voxel_size": VOXEL, "gravity_dim": GRAVITY, "rows": ROWS,
            "feature_keys": "x,heights", "full": FULL, "centre_ulp": STATS["ulp"], "centre_edge": STATS["edge"]}
    print("torch.mean's centre vs the exactly rounded mean: at most", STATS["ulp"], "ulp; nearest rounding boundary (relative)",
          STATS["edge"])
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
