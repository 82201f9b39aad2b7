"""numpy restatements for the ScanNet validation / whole-room test path (tests only): the per-sub-cloud steps of the cloud loop
(examples/segmentation/main_AA.py:84, 584-610 with `test: [PointsToTensor, NumpyChromaticNormalize]`), the val item
(dataset/scannetv2/scannet.py:140-176 after the presampling crop_pc) and the vote in a fixed order.  Pinned to what the
reference's own code returned (tests/golden/scannet_eval.npz) by tests/test_scannet_eval_host.py."""
import numpy as np

COLOR_MEAN = np.array([0.46259782, 0.46253258, 0.46253258]).astype(np.float32)
COLOR_STD = np.array([0.693565, 0.6852543, 0.68061745]).astype(np.float32)
VOXEL = 0.02
U = 2.0 ** -24  # unit roundoff of float32


def make_room(first_id, n_base, copies, seed, dark=False):
    """a raw room in the manner of tests/tools/gen_golden_scannet.py: jittered copies of a synthetic scene off the origin,
    colours in [-1, 1] (dark: every colour <= 1 after (f + 1) * 127.5), labels 0..19 with -100"""
    from amcontrast3d_amd import synthetic
    room = synthetic.make_batch(1, n_base, first_id=first_id, voxel_size=VOXEL)
    rng = np.random.default_rng(seed)
    base = room["pos"][0].astype(np.float32) + np.float32([1.5, -2.0, 0.1])
    coord = np.concatenate([base + rng.uniform(-0.012, 0.012, base.shape).astype(np.float32) for _ in range(copies)], 0)
    feat = np.concatenate([room["x"][0, :3].T] * copies, 0).astype(np.float32) * 2 - 1
    if dark:
        feat = (-1 + (feat + 1) * np.float32(0.5 / 127.5)).astype(np.float32)
    label = np.concatenate([room["y"][0]] * copies, 0).astype(np.int64) % 20
    label[rng.random(len(label)) < 0.05] = -100
    perm = rng.permutation(len(coord))
    return coord[perm].astype(np.float32), feat[perm].astype(np.float32), label[perm]


def stable_tables(shifted, voxel_size=VOXEL):
    """voxelize(mode=1) of dataset/data_util.py:127-143 with a STABLE sort (the reference's own is not): idx_sort, voxel_idx,
    start, count"""
    cells = np.floor(shifted / np.array(voxel_size)).astype(np.uint64)
    key = np.full(cells.shape[0], 14695981039346656037, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(3):
            key *= np.uint64(1099511628211)
            key ^= cells[:, j]
    idx_sort = np.argsort(key, kind="stable")
    _, voxel_idx, count = np.unique(key[idx_sort], return_inverse=True, return_counts=True)
    start = np.cumsum(np.insert(count, 0, 0))
    return idx_sort, voxel_idx.reshape(-1), start, count


def sub_cloud(shifted, feat, idx, mode, gravity_dim=2, color_mean=COLOR_MEAN, color_std=COLOR_STD):
    """one sub-cloud `idx` of the room (coordinates already at the room's min corner, colours as the .pth holds them) ->
    pos (n,3), x (n,3), heights (n,1), all float32"""
    pos = shifted[idx]
    pos = pos - pos.min(0)
    x = feat[idx]
    x = np.clip((x + 1) / 2., 0, 1).astype(np.float32) if mode == "test" else ((x + 1) * 127.5).astype(np.float32)
    if x.max() > 1:
        x = x / 255.
    x = (x - color_mean) / color_std
    assert pos.dtype == np.float32 and x.dtype == np.float32
    return pos, x, pos[:, gravity_dim:gravity_dim + 1]


def assemble(pos, x, heights, feature_keys="pos,x,heights"):
    """get_features_by_keys for one cloud: (Cx, n)"""
    named = {"pos": pos, "x": x, "heights": heights}
    return np.ascontiguousarray(np.concatenate([named[k] for k in feature_keys.split(",")], axis=1).T)


def votes_of(P, start, count, voxel_idx):
    """per SORTED position: rank in its voxel, the voxel's count and the number of parts that hold the point"""
    v = np.asarray(voxel_idx)
    r = np.arange(len(v)) - np.asarray(start)[v]
    c = np.asarray(count)[v]
    return r, c, (P - 1 - r) // c + 1


def vote(logits, where, start, count, idx_sort, voxel_idx, dtype=np.float32):
    """logits (P,C,nvox) -> voted (N,C): per room point the sum over its parts in ASCENDING part order, divided by their
    number, in `dtype` arithmetic (float32: the kernel's own operations; float64: the exact mean to compare against).
    Also returns sum |x_i| per point and class (float64) and the number of votes per point, both in room order."""
    P, C, nvox = logits.shape
    N = len(idx_sort)
    v = np.asarray(voxel_idx)
    r, c, k = votes_of(P, start, count, v)
    acc = np.zeros((N, C), dtype)
    mag = np.zeros((N, C), np.float64)
    for i in range(P):
        m = (i >= r) & ((i - r) % c == 0)
        x = logits[i][:, where[i, v[m]]].T
        acc[m] = acc[m] + x.astype(dtype)
        mag[m] += np.abs(x.astype(np.float64))
    mean = acc / k.astype(dtype)[:, None]
    assert mean.dtype == dtype
    out, out_mag, out_k = np.empty_like(mean), np.empty_like(mag), np.empty(N, np.int64)
    out[idx_sort], out_mag[idx_sort], out_k[idx_sort] = mean, mag, k
    return out, out_mag, out_k


def vote_bound(mag, k):
    """|fl(mean) - mean| <= gamma_k * sum|x_i| / k, gamma_k = k u / (1 - k u): k - 1 additions and one division, each
    rounded once (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)"""
    g = k * U / (1 - k * U)
    return g[:, None] * mag / k[:, None]


def fixture_room(g, tag):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


def fixture_part(room, rows, i):
    """sub-cloud i of the fixture: pos (n,3), x (n,3), heights (n,1), input (7,n)"""
    a = dict(zip(rows, room[f"rows/{i}"]))
    return (np.stack([a["pos0"], a["pos1"], a["pos2"]], 1), np.stack([a["x0"], a["x1"], a["x2"]], 1), a["heights"][:, None],
            np.stack([a[f"in{c}"] for c in range(7)]))


def fixture_perm(room):
    """the reference's shuffles as permutations of the voxel ids, and start"""
    voxel_of = np.empty(len(room["idx_sort"]), np.int64)
    voxel_of[room["idx_sort"]] = room["voxel_idx"]
    return voxel_of[room["parts"]], np.cumsum(np.insert(room["count"], 0, 0))
