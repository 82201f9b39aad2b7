"""numpy restatements for the S3DIS validation / whole-room test path (tests only): `load_data`'s s3dis branch and the
per-sub-cloud steps of the cloud loop (examples/segmentation/main.py:73, 86, 563-587) with `val: [PointsToTensor,
PointCloudXYZAlign, ChromaticNormalize]`, and the val item (dataset/s3dis/s3dis.py:99-144 with presample).  Pinned to what the
reference's own code returned (tests/golden/s3dis_eval.npz) by tests/test_s3dis_eval_host.py.

The one thing the reference leaves open is the last bit of PointCloudXYZAlign's torch.mean (its summation order depends on
the host's vector width and thread count).  `centre` takes it from outside; `exact_centre` is the project's own definition:
the exactly rounded column mean (math.fsum), rounded once to float32."""
import math

import numpy as np

from scannet_eval_ref import U, fixture_room, stable_tables as _stable_tables, vote, vote_bound, votes_of  # noqa: F401

COLOR_MEAN = np.array([0.5136457, 0.49523646, 0.44921124]).astype(np.float32)  # ChromaticNormalize's defaults
COLOR_STD = np.array([0.18308958, 0.18415008, 0.19252081]).astype(np.float32)
VOXEL = 0.06
COORD_SCALE = 2.0 ** -26


def make_raw_room(tag, seed=None):
    """the fixture's raw rooms in their compact exact form (tests/tools/gen_golden_s3dis_eval.py): jittered copies of a
    synthetic scene off the origin, about 6000 points, several points per 6 cm voxel.
    a: float64, coordinates as int32 multiples of 2**-26, colours 0..255;  b: float32, colours k / 255 <= 1 (dark)."""
    from amcontrast3d_amd import synthetic
    first_id, default_seed = {"a": (950, 61), "b": (951, 73)}[tag]
    seed = default_seed if seed is None else seed
    n_base = 1050
    room = synthetic.make_batch(1, n_base, first_id=first_id, voxel_size=VOXEL)
    rng = np.random.default_rng(seed)
    base = room["pos"][0].astype(np.float64) + np.array([3.5, -2.0, 0.25])
    # the copies thin out, so that the voxels hold 1 .. 6 (and, where neighbours spill over, more) points
    keep = [rng.random(n_base) < p for p in (1.0, 1.0, 0.95, 0.9, 0.75, 0.6)]
    coord = np.concatenate([(base + rng.uniform(-0.03, 0.03, base.shape))[k] for k in keep], 0)
    colour = np.concatenate([np.rint(room["x"][0, :3].T * 255)[k] for k in keep], 0).clip(0, 255).astype(np.uint8)
    label = np.concatenate([room["y"][0][k] for k in keep], 0).astype(np.uint8) % 13
    perm = rng.permutation(len(coord))
    coord, colour, label = coord[perm], colour[perm], label[perm]
    out = {"colour_u8": colour, "label_u8": label}
    if tag == "a":
        out["coord_q"] = np.rint(coord / COORD_SCALE).astype(np.int32)
    else:
        out["coord"] = coord.astype(np.float32)
    return out


def fixture_cdata(room):
    """the raw (n,7) array of a room of the fixture, in the dtype of its .npy file"""
    if "coord_q" in room:
        coord = room["coord_q"].astype(np.float64) * COORD_SCALE
        colour = room["colour_u8"].astype(np.float64)
    else:
        coord = room["coord"].astype(np.float32)
        colour = room["colour_u8"].astype(np.float32) / np.float32(255)
    return np.concatenate([coord, colour, room["label_u8"].astype(coord.dtype)[:, None]], 1)


def stable_tables(shifted, voxel_size=VOXEL):
    return _stable_tables(shifted, voxel_size)


def exact_centre(q):
    """(3,) float32: the exact column mean of the float32 array q (n,3), rounded once (NaN for a column that holds one)"""
    out = np.empty(3, np.float32)
    for c in range(3):
        col = q[:, c]
        out[c] = np.float32(np.nan) if np.isnan(col).any() else np.float32(math.fsum(col.tolist()) / len(col))
    return out


def align_normalize(q, x, gravity_dim=2, color_mean=COLOR_MEAN, color_std=COLOR_STD, centre=None):
    """[PointsToTensor, PointCloudXYZAlign, ChromaticNormalize] and the loop's heights on one sub-cloud: q (n,3) the
    coordinates the transforms see (any float dtype), x (n,3) float32 colours -> pos, x, heights, centre, all float32"""
    g = gravity_dim
    with np.errstate(invalid="ignore"):
        heights = q[:, g:g + 1].astype(np.float32)
        pos = q.astype(np.float32)                      # PointsToTensor
        centre = exact_centre(pos) if centre is None else np.asarray(centre, np.float32)
        pos = pos - centre                              # PointCloudXYZAlign
        pos[:, g] = pos[:, g] - pos[:, g].min()
        if x.max() > 1:                                 # ChromaticNormalize
            x = x / np.float32(255.)
        x = (x - color_mean) / color_std
    assert pos.dtype == x.dtype == heights.dtype == np.float32
    return pos, x, heights, centre


def sub_cloud(coord, colour, idx, mode, gravity_dim=2, color_mean=COLOR_MEAN, color_std=COLOR_STD, centre=None):
    """one sub-cloud `idx` of the room -> pos (n,3), x (n,3), heights (n,1), centre (3), all float32.
    coord: already at the room's minimum corner, in the file's dtype (test) or float32 (val); colour: raw, same dtype.
    mode 'test': load_data's colour map and the loop's own min-corner shift, in the file's dtype; 'val': neither."""
    with np.errstate(invalid="ignore"):
        if mode == "test":
            x = np.clip(colour[idx] / 255., 0, 1).astype(np.float32)
            q = coord[idx]
            q = q - q.min(0)
        else:
            assert coord.dtype == np.float32 and colour.dtype == np.float32
            x = colour[idx]
            q = coord[idx]
    return align_normalize(q, x, gravity_dim, color_mean, color_std, centre)


def assemble(pos, x, heights, feature_keys="x,heights"):
    """get_features_by_keys for one cloud: (Cx, n)"""
    named = {"pos": pos, "x": x, "heights": heights}
    return np.ascontiguousarray(np.concatenate([named[k] for k in feature_keys.split(",")], axis=1).T)


def fixture_rows(a, rows):
    """a recorded (len(rows), m) block -> pos (m,3), x (m,3), heights (m,1), input (4,m)"""
    a = dict(zip(rows, a))
    return (np.stack([a["pos0"], a["pos1"], a["pos2"]], 1), np.stack([a["x0"], a["x1"], a["x2"]], 1), a["heights"][:, None],
            np.stack([a[f"in{c}"] for c in range(4)]))


def fixture_perm(room):
    """the reference's shuffles as permutations of the voxel ids, and start"""
    idx_sort, parts = room["idx_sort"].astype(np.int64), room["parts"].astype(np.int64)
    voxel_of = np.empty(len(idx_sort), np.int64)
    voxel_of[idx_sort] = room["voxel_idx"]
    return voxel_of[parts], np.cumsum(np.insert(room["count"].astype(np.int64), 0, 0))


def ulp_distance(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())
