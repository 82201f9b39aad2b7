"""ScanNet's training input for a whole batch of rooms per call (csrc/room_input.hip, input_pipeline.scannet_train_rooms,
input_pipeline.ScanNetTrainFeed): against the per-room route scannet_train_batch on the same draws and against the numpy
restatement (tests/scannet_input_ref.py, pinned to the reference's run by tests/golden/scannet_input.npz), bit for bit: there
are no tolerances here.  The small helpers are those of tests/test_gpu_scannet_input.py."""
import warnings

import numpy as np
import pytest
import torch

import scannet_input_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KWARGS = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
          "color_mean": list(ref.COLOR_MEAN), "color_std": list(ref.COLOR_STD)}  # cfgs/scannet/default.yaml
VOXEL = 0.02
KEYS = ("pos", "x", "heights", "y")


def _aug():
    from amcontrast3d_amd.augment import ScanNetTrainAugment
    return ScanNetTrainAugment(**KWARGS)


def _case(tag):
    g = load_golden("scannet_input")
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


def _draws(rooms_draws, with_R=True):
    """per-room draw dicts (numpy) -> the `draws` argument of scannet_train_batch / scannet_train_rooms"""
    d = {"angle": [r["angle"] for r in rooms_draws], "scale": [float(r["scale"]) for r in rooms_draws],
         "mirror_u": [np.asarray(r["mirror_u"]) for r in rooms_draws], "contrast_u": [r["contrast_u"] for r in rooms_draws],
         "blend": [0.0 if np.isnan(r["blend"]) else r["blend"] for r in rooms_draws], "drop_u": [r["drop_u"] for r in rooms_draws]}
    if with_R:
        d["R"] = [np.asarray(r["R"]) for r in rooms_draws]
    for k in ("rnd", "init_idx", "pad", "perm"):
        d[k] = [None if r.get(k) is None else (torch.as_tensor(np.asarray(r[k])) if k != "init_idx" else int(r[k])) for r in rooms_draws]
    return d


def _fixture_draws(c):
    r = {k: c[k] for k in ("R", "angle", "mirror_u", "contrast_u", "blend", "drop_u", "rnd", "perm")}
    r["scale"] = float(c["scale"][0])
    r["init_idx"] = int(c["init_idx"]) if c["init_idx"] >= 0 else None
    r["pad"] = c["pad"] if len(c["pad"]) else None
    return r


def _gpu_room(coord, feat, label):
    return (torch.from_numpy(np.ascontiguousarray(coord)).to(DEV), torch.from_numpy(np.ascontiguousarray(feat)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(label)).to(DEV))


def _want(coord, feat, label, r, voxel_max, variable=False, voxel=VOXEL):
    pos, x = ref.transform_room(coord, feat, r["R"], r["scale"], r["mirror_u"], r["contrast_u"], r["blend"], r["drop_u"])
    return ref.crop_room(pos, x, label, voxel, voxel_max, variable, r["rnd"], r.get("init_idx"), r.get("pad"), r["perm"])


def _assert_batch(out, wants):
    for b, w in enumerate(wants):
        for k in KEYS:
            np.testing.assert_array_equal(out[k][b].cpu().numpy(), w[k], err_msg=f"room {b}: {k}")
    assert out["pos"].dtype == out["x"].dtype == out["heights"].dtype == torch.float32 and out["y"].dtype == torch.int64


def _assert_same(got, want):
    """two batches equal bit for bit (NaN colours equal NaN colours)"""
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=k)


def _big_room(seed, side=280, spacing=0.022):
    """~157 k raw points: a 6 m lattice floor with a relief, two jittered points per lattice site (2 cm voxels hold
    several points), colours in [-1, 1], labels with -100"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * spacing
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 0.8], len(g))
    base = np.concatenate([g, z[:, None]], 1) + np.array([-3.0, 1.0, 0.2])
    coord = np.concatenate([base + rng.uniform(-0.003, 0.003, base.shape) for _ in range(2)], 0).astype(np.float32)
    feat = rng.uniform(-1, 1, coord.shape).astype(np.float32)
    label = rng.integers(0, 20, len(coord)).astype(np.int64)
    label[rng.random(len(label)) < 0.03] = -100
    return coord, feat, label


def _small_room(seed, n_base=3000, copies=3, label=None):
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(0, 2.0, n_base), rng.uniform(0, 1.5, n_base), rng.choice([0.0, 1.2], n_base) + rng.uniform(0, 0.3, n_base)], 1)
    coord = np.concatenate([base + rng.uniform(-0.008, 0.008, base.shape) for _ in range(copies)], 0).astype(np.float32)
    feat = rng.uniform(-1, 1, coord.shape).astype(np.float32)
    lab = rng.integers(-1, 20, len(coord)).astype(np.int64)
    lab[lab < 0] = -100
    if label is not None:
        lab[:] = label
    return coord, feat, lab


def _room_draws(rng, coord, feat, label, voxel_max, contrast=None, drop=None, variable=False, voxel=VOXEL):
    """draws for one room with the restatement's voxel count (rnd / init / pad / perm need it)"""
    import math
    r = {"angle": float(rng.uniform(-math.pi, math.pi)), "scale": float(rng.uniform(0.8, 1.2)), "mirror_u": rng.random(3),
         "contrast_u": float(rng.random()) if contrast is None else (0.1 if contrast else 0.9), "blend": float(rng.random()),
         "drop_u": float(rng.random()) if drop is None else (0.1 if drop else 0.9)}
    r["R"] = ref.rotation(r["angle"])
    pos, _ = ref.transform_room(coord, feat, r["R"], r["scale"], r["mirror_u"], r["contrast_u"], r["blend"], r["drop_u"])
    p = pos - pos.min(0)
    key = ref.fnv_hash_vec(np.floor(p / np.array(voxel)))
    count = np.unique(key, return_counts=True)[1]
    N = len(count)
    r["rnd"] = rng.integers(0, count.max(), N)
    r["init_idx"] = int(rng.integers(N)) if N >= voxel_max else None
    r["pad"] = rng.integers(0, N, voxel_max - N) if (N < voxel_max and not variable) else None
    r["perm"] = rng.permutation(voxel_max if (N >= voxel_max or not variable) else N)
    return r, N


def _nvox(room, seed):
    """the room's voxel count under the transform draws of default_rng(seed) (the first draws of _room_draws)"""
    return _room_draws(np.random.default_rng(seed), *room, 1)[1]


def _both(rooms, draws, voxel_max, variable=False, voxel=VOXEL):
    """the joint route and the per-room route on the same rooms and draws"""
    from amcontrast3d_amd import input_pipeline as ip
    g = [_gpu_room(*rm) for rm in rooms]
    aug = _aug()
    got = ip.scannet_train_rooms(g, aug, voxel, voxel_max, variable=variable, draws=_draws(draws))
    want = ip.scannet_train_batch(g, aug, voxel, voxel_max, variable=variable, draws=_draws(draws))
    _assert_same(got, want)
    return got


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_rooms_match_the_restatement_and_the_per_room_route(tag):
    c = _case(tag)
    r = _fixture_draws(c)
    vm = int(c["voxel_max"])
    got = _both([(c["coord"], c["feat"], c["label"])], [r], vm)
    _assert_batch(got, [_want(c["coord"], c["feat"], c["label"], r, vm)])


RAGGED = [(31, 3001), (32, 2003), (33, 1499)]  # 9003, 6009 and 4497 points: no multiple of 64


def _ragged(voxel_max_of):
    rooms = [_small_room(seed, n_base=n) for seed, n in RAGGED]
    assert [len(rm[0]) for rm in rooms] == [9003, 6009, 4497] and all(len(rm[0]) % 64 for rm in rooms)
    counts = [_nvox(rm, 100 + i) for i, rm in enumerate(rooms)]
    vm = voxel_max_of(sorted(counts))
    draws = [_room_draws(np.random.default_rng(100 + i), *rm, vm)[0] for i, rm in enumerate(rooms)]
    return rooms, draws, counts, vm


def test_ragged_batch_with_a_cropped_and_a_padded_room():
    rooms, draws, counts, vm = _ragged(lambda s: (s[0] + s[1]) // 2)
    assert min(counts) < vm <= sorted(counts)[1]  # the smallest room is padded, the two others are cropped
    assert draws[counts.index(min(counts))]["pad"] is not None and draws[counts.index(max(counts))]["init_idx"] is not None
    got = _both(rooms, draws, vm)
    assert got["pos"].shape == (3, vm, 3)
    _assert_batch(got, [_want(*rm, r, vm) for rm, r in zip(rooms, draws)])


def test_ragged_batch_where_no_room_crops():
    rooms, draws, counts, vm = _ragged(lambda s: s[2] + 100)
    assert all(r["init_idx"] is None and r["pad"] is not None for r in draws)
    _both(rooms, draws, vm)


def test_ragged_batch_where_every_room_crops():
    rooms, draws, counts, vm = _ragged(lambda s: s[0] - 100)
    assert all(r["init_idx"] is not None for r in draws)
    _both(rooms, draws, vm)


def test_the_same_room_twice_in_a_row():
    """equal keys meet at the room boundary: the boundary still starts a voxel"""
    room, other = _small_room(34, n_base=1499), _small_room(35, n_base=2003)
    n = _nvox(room, 7)
    vm = n - 200
    r = _room_draws(np.random.default_rng(7), *room, vm)[0]
    ro = _room_draws(np.random.default_rng(8), *other, vm)[0]
    twice = _both([room, room], [r, r], vm)
    for k in KEYS:
        np.testing.assert_array_equal(twice[k][0].cpu().numpy(), twice[k][1].cpu().numpy(), err_msg=k)
    once = _both([other, room], [ro, r], vm)
    for k in KEYS:
        np.testing.assert_array_equal(once[k][1].cpu().numpy(), twice[k][0].cpu().numpy(), err_msg=k)
    padded = _both([room, room, other], [_room_draws(np.random.default_rng(7), *room, n + 50)[0]] * 2 +
                   [_room_draws(np.random.default_rng(8), *other, n + 50)[0]], n + 50)
    assert torch.equal(padded["pos"][0], padded["pos"][1]) and torch.equal(padded["y"][0], padded["y"][1])


def _lattice_room(rng):
    """24 x 20 x 3 lattice sites ijk / 32 + (4, 8, 1), exact in fp32, two coincident points per site, shuffled"""
    ijk = np.stack(np.meshgrid(np.arange(24), np.arange(20), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    sites = (ijk * 0.03125 + np.array([4.0, 8.0, 1.0])).astype(np.float32)
    coord = np.concatenate([sites, sites], 0)[rng.permutation(2 * len(sites))]
    feat = rng.uniform(-1, 1, coord.shape).astype(np.float32)
    label = rng.integers(0, 20, len(coord)).astype(np.int64)
    return coord, feat, label


def test_lattice_room_whose_crop_cut_falls_inside_a_float64_tie():
    voxel, vm = 0.03125, 600
    rng = np.random.default_rng(5)
    room = _lattice_room(rng)
    r = {"angle": 0.0, "R": np.eye(3), "scale": 1.0, "mirror_u": np.ones(3), "contrast_u": 0.9, "blend": 0.5, "drop_u": 0.9}
    p = room[0].astype(np.float64) - room[0].astype(np.float64).min(0)
    count = np.unique(ref.fnv_hash_vec(np.floor(p / np.array(voxel))), return_counts=True)[1]
    assert len(count) == 1440 and set(count.tolist()) == {2}
    r["rnd"], r["init_idx"], r["pad"], r["perm"] = rng.integers(0, count.max(), 1440), int(rng.integers(1440)), None, rng.permutation(vm)
    want = _want(*room, r, vm, voxel=voxel)
    d2 = want["d2"]
    cut = np.sort(d2, kind="stable")[vm - 1]
    at_cut, inside = int((d2 == cut).sum()), int((d2[want["crop_idx"]] == cut).sum())
    print("lattice: distinct distances", len(np.unique(d2)), "- representatives at the cut distance", at_cut, "- inside the crop", inside)
    assert len(np.unique(d2)) == 413 and at_cut == 10 and inside == 5  # the cut falls inside a tie: the stable order decides
    other = _small_room(36, n_base=1499)
    ro = _room_draws(np.random.default_rng(9), *other, vm, voxel=voxel)[0]
    got = _both([room, other], [r, ro], vm, voxel=voxel)
    _assert_batch(got, [want, _want(*other, ro, vm, voxel=voxel)])
    got = _both([other, room], [ro, r], vm, voxel=voxel)
    _assert_batch(got, [_want(*other, ro, vm, voxel=voxel), want])


def test_exactly_voxel_max_voxels_and_a_single_room():
    room, other = _small_room(37, n_base=1499), _small_room(38, n_base=2003)
    vm = _nvox(room, 11)  # a crop that keeps everything, in distance order
    r = _room_draws(np.random.default_rng(11), *room, vm)[0]
    assert r["init_idx"] is not None and r["pad"] is None
    want = _want(*room, r, vm)
    assert len(want["crop_idx"]) == vm == len(want["idx_unique"])
    got = _both([room], [r], vm)  # B = 1: no room bits, one sort each
    _assert_batch(got, [want])
    ro = _room_draws(np.random.default_rng(12), *other, vm)[0]
    got = _both([other, room], [ro, r], vm)
    _assert_batch(got, [_want(*other, ro, vm), want])


def test_nan_colours_stay_in_their_own_room():
    coord, feat, label = _small_room(39, n_base=1499)
    feat[:, 1] = 0.25  # hi == lo with contrast taken: numpy's NaN (test_edge_constant_colour_channel_with_contrast_gives_numpys_nan)
    other = _small_room(40, n_base=2003)
    vm = 3000
    r = _room_draws(np.random.default_rng(13), coord, feat, label, vm, contrast=True, drop=False)[0]
    ro = _room_draws(np.random.default_rng(14), *other, vm, contrast=True, drop=False)[0]
    got = _both([(coord, feat, label), other], [r, ro], vm)
    x = got["x"].cpu().numpy()
    assert np.all(np.isnan(x[0, :, 1])) and not np.any(np.isnan(x[0][:, [0, 2]])) and not np.any(np.isnan(x[1]))
    assert bool(torch.isfinite(got["pos"]).all())
    _assert_batch(got, [_want(coord, feat, label, r, vm), _want(*other, ro, vm)])


def test_variable_rooms():
    from amcontrast3d_amd import input_pipeline as ip
    room = _small_room(41, n_base=1499)
    r, n = _room_draws(np.random.default_rng(15), *room, 100000, variable=True)
    got = _both([room], [r], 100000, variable=True)  # no crop, no padding: the room's own voxel count
    assert got["pos"].shape == (1, n, 3) and n < 100000
    _assert_batch(got, [_want(*room, r, 100000, variable=True)])
    with pytest.raises(ValueError):  # the collate stacks: rooms of different sizes cannot form one batch
        ip.scannet_train_rooms([_gpu_room(*room), _gpu_room(*_small_room(42, n_base=2003))], _aug(), VOXEL, 100000, variable=True,
                               generator=torch.Generator(device=DEV).manual_seed(0))


def test_generator_runs_are_reproducible_and_rooms_stay_apart():
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu_room(*_small_room(43 + b, n_base=n, label=b)) for b, (_, n) in enumerate(RAGGED)]
    aug = _aug()
    vm = 3500  # whatever the rotation and scale, room 0 (about 5500 to 6500 voxels) is cropped and room 2 (2750 to 3300) padded
    runs = [ip.scannet_train_rooms(rooms, aug, VOXEL, vm, generator=torch.Generator(device=DEV).manual_seed(7)) for _ in range(2)]
    _assert_same(runs[0], runs[1])
    other = ip.scannet_train_rooms(rooms, aug, VOXEL, vm, generator=torch.Generator(device=DEV).manual_seed(8))
    assert not torch.equal(runs[0]["pos"], other["pos"])
    out = runs[0]
    assert out["pos"].shape == (3, vm, 3) and out["heights"].shape == (3, vm, 1) and out["y"].shape == (3, vm)
    assert bool(torch.isfinite(out["pos"]).all())
    for b in range(3):  # every label is a label of its own room
        assert bool((out["y"][b] == b).all())
    assert torch.equal(out["pos"].amin(dim=1), torch.zeros(3, 3, device=DEV))  # every cloud sits at its own min corner
    assert torch.equal(out["heights"].amin(dim=(1, 2)), torch.zeros(3, device=DEV))
    assert torch.equal(out["heights"][..., 0], out["pos"][..., 2])


def _sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return [w for w in seen if "synchroniz" in str(w.message).lower()]


def test_one_read_back_per_batch():
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu_room(*_small_room(50 + b, n_base=n)) for b, (_, n) in enumerate(RAGGED)]
    aug = _aug()
    gen = torch.Generator(device=DEV).manual_seed(1)
    host = aug.draw(3)  # the room-level draws as host values; the crop draws come from the device generator
    per_room = lambda: ip.scannet_train_batch(rooms, aug, VOXEL, 3500, generator=gen, draws=dict(host))  # noqa: E731
    joint = lambda: ip.scannet_train_rooms(rooms, aug, VOXEL, 3500, generator=gen, draws=dict(host))  # noqa: E731
    feed = ip.ScanNetTrainFeed(rooms, aug, batch_size=3, loop=4, voxel_max=3500, generator=gen)
    running = iter(feed)
    per_room(), joint(), next(running)  # warm: constants uploaded, code objects loaded, the epoch's draws made
    n_room = len(_sync_warnings(per_room))
    if n_room < 1:
        pytest.skip("this build raises no synchronisation warning for scannet_train_batch's read-backs")
    got = _sync_warnings(joint)
    from_feed = _sync_warnings(lambda: next(running))
    print("synchronisation warnings for three rooms: scannet_train_batch", n_room, "- scannet_train_rooms", len(got),
          "- one batch of a running ScanNetTrainFeed", len(from_feed))
    assert len(got) <= 1, [str(w.message) for w in got]
    assert len(from_feed) <= 1, [str(w.message) for w in from_feed]


def test_full_size_batch():
    rng = np.random.default_rng(7)
    rooms = [_big_room(1), _big_room(2)]
    draws = []
    for i, room in enumerate(rooms):
        r, N = _room_draws(rng, *room, 64000, contrast=(i == 0), drop=False)
        assert N >= 64000 and len(room[0]) > 140000
        draws.append(r)
    got = _both(rooms, draws, 64000)
    assert got["pos"].shape == (2, 64000, 3) and got["heights"].shape == (2, 64000, 1) and got["y"].shape == (2, 64000)


def test_errors():
    from amcontrast3d_amd import input_pipeline as ip
    aug = _aug()
    room_np = _small_room(60, n_base=1499)
    room = _gpu_room(*room_np)
    N = _nvox(room_np, 17)
    ok = _room_draws(np.random.default_rng(17), *room_np, N - 100)[0]
    base = _draws([ok])

    def bad(rooms, vm=N - 100, **over):
        d = {k: v for k, v in base.items() if k not in ("rnd", "init_idx", "pad", "perm")}
        d.update(over)
        return ip.scannet_train_rooms(rooms, aug, VOXEL, vm, generator=torch.Generator(device=DEV).manual_seed(0), draws=d)
    with pytest.raises(ValueError):
        ip.scannet_train_rooms([], aug, VOXEL, 1000)
    with pytest.raises(RuntimeError):
        bad([tuple(t.cpu() for t in room)])
    with pytest.raises(RuntimeError):
        bad([(room[0].double(), room[1], room[2])])
    with pytest.raises(ValueError):
        bad([(room[0][:-1], room[1], room[2])])
    with pytest.raises(ValueError):
        bad([room], vm=None)
    for key in ("rnd", "init_idx", "pad", "perm"):
        with pytest.raises(ValueError):
            bad([room], **{key: [None, None]})  # one entry per room
    for key, value in (("rnd", ok["rnd"][:-1]), ("rnd", -1 - ok["rnd"]), ("init_idx", N), ("init_idx", -1),
                       ("perm", ok["perm"][:-1]), ("perm", np.zeros_like(ok["perm"]))):
        with pytest.raises(ValueError):
            bad([room], **{key: [torch.from_numpy(value) if isinstance(value, np.ndarray) else value]})
    for value in (np.zeros(99, dtype=np.int64), np.full(100, N, dtype=np.int64)):  # N + 100 slots: 100 padding draws below N
        with pytest.raises(ValueError):
            bad([room], vm=N + 100, pad=[torch.from_numpy(value)])
    out = bad([room], rnd=[torch.from_numpy(ok["rnd"])], init_idx=[ok["init_idx"]], perm=[torch.from_numpy(ok["perm"])])
    _assert_batch(out, [_want(*room_np, ok, N - 100)])


def _feed(n_rooms=3, **kw):
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu_room(*_small_room(70 + b, n_base=1499 + 251 * b, label=b)) for b in range(n_rooms)]
    return ip.ScanNetTrainFeed(rooms, _aug(), **kw)


def _visited(batches):
    for b in batches:  # a cloud's labels are its room's
        assert bool((b["y"] == b["y"][:, :1]).all())
    return [int(v) for b in batches for v in b["y"][:, 0].tolist()]


def test_feed_len_and_unshuffled_order():
    gen = torch.Generator(device=DEV).manual_seed(3)
    feed = _feed(batch_size=2, loop=3, voxel_max=2048, shuffle=False, generator=gen)
    assert len(feed) == 4
    batches = list(feed)
    assert len(batches) == 4 and all(b["pos"].shape == (2, 2048, 3) and b["heights"].shape == (2, 2048, 1) for b in batches)
    assert _visited(batches) == [i % 3 for i in range(8)]  # item id -> room id % len(rooms), the ninth item dropped
    feed = _feed(batch_size=2, loop=3, voxel_max=2048, shuffle=False, drop_last=False, generator=gen)
    assert len(feed) == 5
    batches = list(feed)
    assert [b["pos"].shape[0] for b in batches] == [2, 2, 2, 2, 1] and _visited(batches) == [i % 3 for i in range(9)]


def test_feed_shuffled_epochs():
    feed = _feed(batch_size=2, loop=2, voxel_max=2048, generator=torch.Generator(device=DEV).manual_seed(2))
    assert len(feed) == 3
    epochs = []
    for _ in range(2):
        batches = list(feed)
        assert len(batches) == 3
        ids = _visited(batches)
        assert sorted(ids) == [0, 0, 1, 1, 2, 2]  # every room exactly `loop` times
        epochs.append((ids, batches))
    # the second epoch from the same generator: other draws
    assert not all(torch.equal(a["pos"], b["pos"]) for a, b in zip(epochs[0][1], epochs[1][1]))
    again = _feed(batch_size=2, loop=2, voxel_max=2048, generator=torch.Generator(device=DEV).manual_seed(2))
    for e in range(2):  # the same seed: the same two epochs
        batches = list(again)
        assert _visited(batches) == epochs[e][0]
        for a, b in zip(batches, epochs[e][1]):
            _assert_same(a, b)


def test_two_training_iterations_on_feed_batches():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    import openpoints.utils as ou
    from amcontrast3d_amd import configs, input_pipeline as ip, train
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    c = EasyConfig(); c.update(configs.model_cfg("S", num_classes=20, in_channels=7, dropout=0, width=16))
    model = build_model_from_cfg(c).to(DEV)
    cc = EasyConfig(); cc.update(configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    cfg = EasyConfig()
    cfg.update({"num_classes": 20, "ignore_index": -100, "ambiguity_args": configs.ambiguity_args("scannet"),
                "feature_keys": "pos,x,heights", "use_amp": False, "step_per_update": 1, "grad_norm_clip": 10,
                "sched_on_epoch": True})
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    rooms = [_gpu_room(*_small_room(80 + b)) for b in range(4)]
    feed = ip.ScanNetTrainFeed(rooms, _aug(), batch_size=2, voxel_max=4096, generator=torch.Generator(device=DEV).manual_seed(5))
    assert len(feed) == 2
    labels = []

    class Seen:
        def __iter__(self):
            for b in feed:
                labels.append(b["y"].clone())
                yield b
    made = []
    real = ou.ConfusionMatrix

    class Recording(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    ou.ConfusionMatrix = Recording
    try:
        got = train.train_one_epoch(model, Seen(), crit, opt, None, None, 1, cfg)
    finally:
        ou.ConfusionMatrix = real
    assert np.isfinite(got[0])
    assert len(labels) == 2 and all(y.shape == (2, 4096) for y in labels)
    assert len(made) == 1 and int(made[0].value.sum()) == sum(int((y != -100).sum()) for y in labels)
