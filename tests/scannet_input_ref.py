"""Plain-numpy restatement of ScanNet's training input (dataset/scannetv2/scannet.py:140-176): colours (feat + 1) * 127.5,
the chain RandomRotateZ, RandomScale, ChromaticAutoContrast, RandomDropFeature, NumpyChromaticNormalize
(transforms/point_transform_cpu.py:43-92,192-209,304-332) on the whole raw room, then crop_pc (dataset/data_util.py:146-174)
and `heights` -- with the random draws given explicitly.  No reference import and no scipy: it runs wherever the tests run.
Pinned to the reference by tests/golden/scannet_input.npz (tests/test_scannet_input_oracle.py).

The one deliberate difference from the reference: the sorts are STABLE (numpy's default argsort is not, so the order of
the points inside one voxel, and of equidistant points in the crop, is not specified by the reference)."""
import numpy as np

COLOR_MEAN = (0.46259782, 0.46253258, 0.46253258)  # cfgs/scannet/default.yaml datatransforms.kwargs
COLOR_STD = (0.693565, 0.6852543, 0.68061745)


def rotation(angle):
    """RandomRotateZ.M(e_z, angle) from cos / sin (the reference uses scipy.linalg.expm: within a dozen ulp of this)"""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def fnv_hash_vec(arr):
    arr = arr.astype(np.uint64)
    h = np.full(arr.shape[0], 14695981039346656037, dtype=np.uint64)
    for j in range(arr.shape[1]):
        h *= np.uint64(1099511628211)
        h ^= arr[:, j]
    return h


def transform_room(coord, feat, R, scale, mirror_u, contrast_u, blend, drop_u, p=0.2, feature_drop=0.2,
                   mirror=(0.2, -1, -1), color_mean=COLOR_MEAN, color_std=COLOR_STD):
    """coord (n,3) f32, feat (n,3) f32 in [-1, 1] -> (pos (n,3) float64, x (n,3) float32), numpy's arithmetic"""
    x = ((feat + 1) * 127.5).astype(np.float32)
    pos = np.dot(coord.astype(np.float32), np.asarray(R, dtype=np.float64))
    sc = np.array([scale], dtype=np.float64).repeat(3) if np.ndim(scale) == 0 else np.array(scale, dtype=np.float64)
    if np.sum(np.array(mirror) > 0) != 0:
        sc *= (np.asarray(mirror_u) > np.array(mirror)).astype(np.float32) * 2 - 1
    pos *= sc
    if contrast_u < p:
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.min(x, 0, keepdims=True)
            hi = np.max(x, 0, keepdims=True)
            cf = (x - lo) * (255 / (hi - lo))
            x = (1 - float(blend)) * x + float(blend) * cf
    if drop_u < feature_drop:
        x[:, 0:3] = 0
    if x.max() > 1:
        x /= 255.
    if color_mean is not None:
        x = (x - np.array(color_mean).astype(np.float32)) / np.array(color_std).astype(np.float32)
    return pos, x


def crop_room(pos, x, y, voxel_size, voxel_max, variable, rnd, init_idx=None, pad=None, perm=None, pick=None, crop=None):
    """crop_pc(..., 'train', voxel_size, voxel_max, variable=variable) on the transformed room with the given draws ->
    dict of the intermediate and final quantities.  `pick` / `crop`: use these idx_unique / crop_idx instead of the
    stable sorts' (to follow a run of the reference, whose unstable sorts may order ties otherwise)."""
    coord = pos - pos.min(0)
    key = fnv_hash_vec(np.floor(coord / np.array(voxel_size)))
    idx_sort = np.argsort(key, kind="stable")
    _, count = np.unique(key[idx_sort], return_counts=True)
    start = np.cumsum(np.insert(count, 0, 0)[0:-1])
    idx_unique = idx_sort[start + np.asarray(rnd) % count] if pick is None else np.asarray(pick)
    cv = coord[idx_unique]
    N = len(idx_unique)
    out = {"key": key, "count": count, "idx_unique": idx_unique}
    crop_idx = None
    if N >= voxel_max:
        d2 = np.sum(np.square(cv - cv[init_idx]), 1)
        crop_idx = np.argsort(d2, kind="stable")[:voxel_max] if crop is None else np.asarray(crop)
        out["d2"], out["crop_idx"] = d2, crop_idx
    elif not variable:
        crop_idx = np.hstack([np.arange(N), np.asarray(pad)])
    crop_idx = np.arange(N) if crop_idx is None else crop_idx
    if perm is not None:
        crop_idx = crop_idx[np.asarray(perm)]
    c = cv[crop_idx]
    c -= c.min(0)
    out["pos"] = c.astype(np.float32)
    out["x"] = x[idx_unique][crop_idx].astype(np.float32)
    out["y"] = np.asarray(y).reshape(-1)[idx_unique][crop_idx].astype(np.int64)
    out["heights"] = out["pos"][:, 2:3] - out["pos"][:, 2:3].min()
    return out
