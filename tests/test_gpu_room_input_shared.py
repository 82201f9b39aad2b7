"""The two instantiations of csrc/room_input.hip on one cloud: the S3DIS entry points (fp32 coordinates, rows of a (rows,7)
raw array) and the ScanNet entry points (fp64 coordinates, a dense (total,3) array) are given the same three rooms, the same
voxel size and the same rnd / init_idx / pad / perm tables, and must agree bit for bit on every table they produce.

The input makes fp32 and fp64 arithmetic coincide exactly: every coordinate is a multiple of 2^-6 below 8, so are the
differences to the min corner and to the crop centre; a squared distance is a sum of three integers below 2^16 in units of
2^-12, far inside fp32's 24 bits; the voxel size 1/16 is a power of two, so the division is exact.  There are no tolerances.

Rooms 0 and 1 (4000 and 1500 points) have at least voxel_max = 1000 voxels and are cropped -- with many equal distances, which
the stable sorts of both instantiations (one pass over (room << 32) | bits for fp32, two passes for fp64) must break alike;
room 2 (700 points) has fewer and is padded."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = (4000, 1500, 700)
VOXEL, VOXEL_MAX, GRAVITY = 1.0 / 16, 1000, 2
SHIFT = np.array([1.5, 2.25, 0.5])  # room 0's min corner is not the origin; a multiple of 2^-6, every value stays below 8


def _cloud():
    rng = np.random.default_rng(7)
    xyz = rng.integers(0, [256, 256, 128], (sum(SIZES), 3)).astype(np.float64) / 64  # [0,4) x [0,4) x [0,2), duplicates allowed
    xyz[:SIZES[0]] += SHIFT
    assert xyz.max() < 8 and np.array_equal(xyz * 64, np.round(xyz * 64))
    raw = np.concatenate([xyz, rng.integers(0, 256, (len(xyz), 3)), rng.integers(0, 13, (len(xyz), 1))], 1).astype(np.float32)
    return xyz, raw


def _voxels_numpy(xyz):
    """distinct occupied cells of every room"""
    off = np.concatenate([[0], np.cumsum(SIZES)])
    return [len(np.unique(np.floor((xyz[a:b] - xyz[a:b].min(0)) / VOXEL), axis=0)) for a, b in zip(off[:-1], off[1:])]


def _run(lib, which, xyz, raw, tables):
    """voxelise, select / crop and tail of one instantiation -> its tables as numpy arrays; `tables` (rnd, init, pad, perm) is
    None on the first run, which then draws them from the voxel counts it reads back"""
    from amcontrast3d_amd import _lib
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    B, total, s3dis = len(SIZES), sum(SIZES), which == "s3dis"
    ctype = torch.float32 if s3dis else torch.float64
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    off_t = up(np.concatenate([[0], np.cumsum(SIZES)]), torch.int64)
    src_t = off_t[:B].clone()
    raw_t, pos_t = up(raw, torch.float32), up(xyz, torch.float64)
    coord = torch.empty(total, 3, dtype=ctype, device=DEV)
    key = torch.empty(total, dtype=torch.int64, device=DEV)
    idx_sort = torch.empty(total, dtype=torch.int32, device=DEV)
    start = torch.empty(total + 1, dtype=torch.int32, device=DEV)
    count = torch.empty(total, dtype=torch.int32, device=DEV)
    vbase = torch.empty(B + 1, dtype=torch.int32, device=DEV)
    cmax = torch.empty(B, dtype=torch.int32, device=DEV)
    corner = torch.empty(B, 3, dtype=ctype, device=DEV)
    wb = int(getattr(lib, f"amc3d_{which}_voxelize_workspace_bytes")(B, total))
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    tabs = (P(coord), P(key), P(idx_sort), P(start), P(count), P(vbase), P(cmax), P(corner), P(work), wb, None)
    if s3dis:
        rc = lib.amc3d_s3dis_voxelize_rooms(B, total, 0, P(raw_t), P(src_t), P(off_t), ctypes.c_double(VOXEL), *tabs)
    else:
        rc = lib.amc3d_scannet_voxelize_rooms(B, total, P(pos_t), P(off_t), ctypes.c_double(VOXEL), *tabs)
    _lib.check(rc, f"{which}_voxelize_rooms")
    vb = vbase.tolist()
    nvt = vb[B]
    if tables is None:
        rng = np.random.default_rng(11)
        nv = np.diff(vb)
        init = np.array([rng.integers(n) if n >= VOXEL_MAX else -1 for n in nv])
        pad = np.stack([rng.integers(0, n, VOXEL_MAX) for n in nv])
        perm = np.stack([rng.permutation(VOXEL_MAX) for _ in nv])
        tables = {"rnd": rng.integers(0, 1000, nvt), "init": init, "pad": pad, "perm": perm}
    rnd, init, pad, perm = (up(tables[k], torch.int32) for k in ("rnd", "init", "pad", "perm"))
    assert rnd.numel() == nvt
    sel = torch.empty(nvt, dtype=torch.int32, device=DEV)
    d2 = torch.empty(nvt, dtype=ctype, device=DEV)
    order = torch.empty(nvt, dtype=torch.int32, device=DEV)
    wb2 = int(getattr(lib, f"amc3d_{which}_crop_workspace_bytes")(nvt))
    work2 = torch.empty(wb2, dtype=torch.uint8, device=DEV)
    _lib.check(getattr(lib, f"amc3d_{which}_select_crop")(B, nvt, VOXEL_MAX, 1, P(coord), P(idx_sort), P(start), P(count), P(vbase),
                                                          P(cmax), P(rnd), None, P(init), None, P(sel), P(d2), P(order), P(work2),
                                                          wb2, None), f"{which}_select_crop")
    pos = torch.empty(B, VOXEL_MAX, 3, dtype=torch.float32, device=DEV)
    feat = torch.empty(B, VOXEL_MAX, 3, dtype=torch.float32, device=DEV)
    y = torch.empty(B, VOXEL_MAX, dtype=torch.int64, device=DEV)
    if s3dis:
        rc = lib.amc3d_s3dis_crop_tail(B, VOXEL_MAX, VOXEL_MAX, 0, P(raw_t), P(src_t), P(off_t), P(coord), P(vbase), P(sel),
                                       P(order), P(pad), P(perm), P(pos), P(feat), P(y), None)
    else:
        x_t, y_t = raw_t[:, 3:6].contiguous(), raw_t[:, 6].long()
        heights = torch.empty(B, VOXEL_MAX, 1, dtype=torch.float32, device=DEV)
        wb3 = int(lib.amc3d_scannet_crop_tail_workspace_bytes(B))
        work3 = torch.empty(wb3 // 8, dtype=torch.float64, device=DEV)
        rc = lib.amc3d_scannet_crop_tail_rooms(B, VOXEL_MAX, VOXEL_MAX, GRAVITY, P(coord), P(x_t), P(y_t), P(vbase), P(sel),
                                               P(order), P(pad), P(perm), P(pos), P(feat), P(heights), P(y), P(work3), wb3, None)
    _lib.check(rc, f"{which}_crop_tail")
    torch.cuda.synchronize()
    out = {"key": key, "idx_sort": idx_sort, "start": start[:nvt + 1], "count": count[:nvt], "vbase": vbase, "cmax": cmax,
           "corner": corner, "coord": coord, "sel": sel, "order": order, "d2": d2, "pos": pos, "x": feat, "y": y}
    return {k: v.cpu().numpy() for k, v in out.items()}, tables


@pytest.fixture(scope="module")
def both():
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    xyz, raw = _cloud()
    with torch.cuda.device(DEV):
        s3dis, tables = _run(lib, "s3dis", xyz, raw, None)
        scannet, _ = _run(lib, "scannet", xyz, raw, tables)
    return xyz, s3dis, scannet


def test_rooms_cover_crop_and_pad(both):
    xyz, s3dis, _ = both
    nv = np.diff(s3dis["vbase"])
    assert nv[0] >= VOXEL_MAX and nv[1] >= VOXEL_MAX and 0 < nv[2] < VOXEL_MAX, nv
    assert list(nv) == _voxels_numpy(xyz)  # the hash merges no two of these cells
    assert s3dis["corner"][0].tolist() == xyz[:SIZES[0]].min(0).tolist() and xyz[:SIZES[0]].min(0).min() > 0
    for r in (0, 1):  # equal distances in both cropped rooms: their order is the stable sorts' tie-break
        d = s3dis["d2"][s3dis["vbase"][r]:s3dis["vbase"][r + 1]]
        assert len(np.unique(d)) < len(d)


@pytest.mark.parametrize("name", ["key", "idx_sort", "start", "count", "vbase", "cmax"])
def test_voxel_tables_agree(both, name):
    _, s3dis, scannet = both
    assert s3dis[name].dtype == scannet[name].dtype
    np.testing.assert_array_equal(s3dis[name], scannet[name])


def test_coord_and_corner_agree(both):
    _, s3dis, scannet = both
    for k in ("coord", "corner"):
        assert s3dis[k].dtype == np.float32 and scannet[k].dtype == np.float64
        np.testing.assert_array_equal(s3dis[k].astype(np.float64), scannet[k])


def test_select_agrees(both):
    _, s3dis, scannet = both
    np.testing.assert_array_equal(s3dis["sel"], scannet["sel"])


def test_crop_agrees(both):
    _, s3dis, scannet = both
    assert s3dis["d2"].dtype == np.float32 and scannet["d2"].dtype == np.float64
    np.testing.assert_array_equal(s3dis["d2"].astype(np.float64), scannet["d2"])
    np.testing.assert_array_equal(s3dis["order"], scannet["order"])


def test_tail_agrees(both):
    _, s3dis, scannet = both
    for k in ("pos", "x", "y"):
        assert s3dis[k].dtype == scannet[k].dtype
        np.testing.assert_array_equal(s3dis[k], scannet[k])
