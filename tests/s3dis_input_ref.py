"""Plain-numpy restatement of one S3DIS training item with presample=False (dataset/s3dis/s3dis.py:122-144): the raw room cast
to float32, xyz -= min, crop_pc (dataset/data_util.py:146-174: min-corner shift, voxelize mode 0, nearest-voxel_max crop or
padding by repetition, shuffle, min-corner shift, cast), the training transform chain of cfgs/s3dis/default.yaml
(oracle/augment_ref.py) and `heights` -- with every random draw given explicitly.  Pinned to the reference by
tests/golden/s3dis_input.npz (tests/test_s3dis_input_oracle.py).

The one deliberate difference from the reference: the sorts are STABLE (numpy's default argsort is not, so the order of the
points inside one voxel, and of equidistant representatives in the crop, is not specified by the reference).  `idx_unique` /
`crop_idx` replace the stable sorts' picks with given ones, to follow a run of the reference."""
import numpy as np

from oracle import augment_ref, input_ref

VOXEL = 0.04
TRANSFORM_KEYS = ("contrast", "blend", "scale_u", "theta", "noise", "drop")


def crop_item(cdata, d, voxel_size=VOXEL, voxel_max=24000, variable=False, shuffle=True, idx_unique=None, crop_idx=None):
    """cdata (n,7) raw room, float32 or float64: xyz, rgb 0..255, label.  d: 'rnd' (nvox), 'init_idx' (N >= voxel_max), 'pad'
    (voxel_max - N, for N < voxel_max and not variable), 'perm'.  -> dict: key, count, idx_unique, [d2, crop_idx,] pos0 (the
    cropped cloud at its min corner, float32), x0 (its raw colours, float32), y (int64)"""
    c = np.asarray(cdata).astype(np.float32)
    c[:, :3] -= np.min(c[:, :3], 0)                    # s3dis.py:129-130
    coord, feat, label = c[:, :3], c[:, 3:6], c[:, 6]
    coord = coord - coord.min(0)                       # data_util.py:151 (the minimum is exactly 0 by now)
    key = input_ref.fnv_hash_vec(np.floor(coord / np.array(voxel_size)))
    idx_sort = np.argsort(key, kind="stable")
    _, count = np.unique(key[idx_sort], return_counts=True)
    start = np.cumsum(np.insert(count, 0, 0)[0:-1])
    pick = idx_sort[start + np.asarray(d["rnd"]) % count] if idx_unique is None else np.asarray(idx_unique)
    cv = coord[pick]
    N = len(pick)
    out = {"key": key, "count": count, "idx_unique": pick}
    idx = np.arange(N)
    if N >= voxel_max:
        d2, stable = input_ref.crop_nearest(cv, int(d["init_idx"]), voxel_max)
        idx = stable if crop_idx is None else np.asarray(crop_idx)
        out["d2"], out["crop_idx"] = d2, idx
    elif not variable:
        idx = np.hstack([idx, np.asarray(d["pad"], dtype=np.int64)])
    if shuffle:
        idx = idx[np.asarray(d["perm"])]
    pos0 = cv[idx]
    pos0 = pos0 - pos0.min(0)                          # data_util.py:173
    out["pos0"] = pos0.astype(np.float32)
    out["x0"] = feat[pick][idx].astype(np.float32)
    out["y"] = label[pick][idx].astype(np.int64)
    return out


def train_item(cdata, d, voxel_size=VOXEL, voxel_max=24000, variable=False, shuffle=True, idx_unique=None, crop_idx=None,
               gravity_dim=2):
    """crop_item, then the transform chain with the draws d[k], k in TRANSFORM_KEYS (one cloud's: scale_u (3), theta (3), noise
    (N,3)); adds pos, x (N,3) and heights (N,1) = the gravity column of pos0"""
    out = crop_item(cdata, d, voxel_size, voxel_max, variable, shuffle, idx_unique, crop_idx)
    t = {"contrast": bool(d["contrast"]), "blend": float(d["blend"]), "scale_u": np.asarray(d["scale_u"]),
         "theta": np.asarray(d["theta"]), "noise": np.asarray(d["noise"]), "drop": bool(d["drop"])}
    out["pos"], out["x"], out["heights"] = augment_ref.s3dis_train(out["pos0"].copy(), out["x0"].copy(), t, gravity_dim=gravity_dim)
    return out
