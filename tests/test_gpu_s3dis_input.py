"""S3DIS training input on the device for a batch of raw rooms (csrc/room_input.hip, input_pipeline.s3dis_train_batch,
input_pipeline.S3DISTrainFeed): against what the reference's own S3DIS.__getitem__ returned for the same raw rooms and draws
(tests/golden/s3dis_input.npz, through the numpy restatement tests/s3dis_input_ref.py), and bit for bit against the per-room
route -- input_pipeline.crop_pc on the shifted float32 room, torch.stack, augment.S3DISTrainAugment -- on the same draws."""
import warnings

import numpy as np
import pytest
import torch

import s3dis_input_ref as ref
from conftest import load_golden
from oracle import input_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VOXEL = 0.04
KEYS = ("pos", "x", "heights", "y")


def _aug():
    from amcontrast3d_amd.augment import S3DISTrainAugment
    return S3DISTrainAugment(color_drop=0.2, gravity_dim=2, scale=[0.9, 1.1], angle=[0, 0, 1], jitter_sigma=0.005,
                             jitter_clip=0.02)  # cfgs/s3dis/default.yaml


def _room(seed, n, label=None, extent=(2.0, 1.5)):
    """a raw room (n,7) float64: three jittered copies of a two-level scene (several points per 4 cm voxel), away from the
    origin; colours 0..255, labels 0..12 (or all `label`)"""
    rng = np.random.default_rng(seed)
    nb = -(-n // 3)
    base = np.stack([rng.uniform(0, extent[0], nb), rng.uniform(0, extent[1], nb),
                     rng.choice([0.0, 1.2], nb) + 0.2 * np.sin(3 * rng.uniform(0, 1, nb))], 1) + np.array([21.5, -3.25, 0.7])
    xyz = np.concatenate([base + rng.uniform(-0.015, 0.015, base.shape) for _ in range(3)], 0)[:n]
    rgb = rng.integers(0, 256, (n, 3)).astype(np.float64)
    lab = rng.integers(0, 13, n).astype(np.float64) if label is None else np.full(n, float(label))
    return np.concatenate([xyz, rgb, lab[:, None]], 1)[rng.permutation(n)]


def _counts(cdata, voxel=VOXEL):
    """points per voxel of the room, as the item sees it (float32 cast, min-corner shift)"""
    c = cdata[:, :3].astype(np.float32)
    c = c - c.min(0)
    return np.unique(input_ref.fnv_hash_vec(np.floor(c / np.array(voxel))), return_counts=True)[1]


def _crop_draws(rng, cdata, voxel_max, voxel=VOXEL):
    count = _counts(cdata, voxel)
    N = len(count)
    return {"rnd": rng.integers(0, count.max(), N), "init_idx": int(rng.integers(N)) if N >= voxel_max else None,
            "pad": rng.integers(0, N, voxel_max - N) if N < voxel_max else None, "perm": rng.permutation(voxel_max)}


def _transform_draws(rng, B, n, contrast=None, drop=None):
    theta = np.zeros((B, 3))
    theta[:, 2] = rng.uniform(-np.pi, np.pi, B)
    d = {"contrast": np.array([bool(b % 2 == 0) for b in range(B)] if contrast is None else contrast),
         "blend": rng.random(B).astype(np.float32), "scale_u": rng.random((B, 3)).astype(np.float32), "theta": theta,
         "noise": rng.standard_normal((B, n, 3)).astype(np.float32),
         "drop": np.array([bool(b % 3 == 2) for b in range(B)] if drop is None else drop)}
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


def _all_draws(crop, t):
    d = dict(t)
    for k in ("rnd", "init_idx", "pad", "perm"):
        d[k] = [None if c[k] is None else (c[k] if k == "init_idx" else torch.from_numpy(np.asarray(c[k]))) for c in crop]
    return d


def _per_room(rooms, aug, voxel_max, crop, t, voxel=VOXEL):
    """the parent route: S3DIS.__getitem__'s cast and shift in torch, crop_pc per room, the collate, the batch transform"""
    from amcontrast3d_amd import input_pipeline as ip
    pos, col, ys = [], [], []
    for room, c in zip(rooms, crop):
        cd = room.float()
        coord = cd[:, :3] - cd[:, :3].min(0).values
        kw = {k: torch.from_numpy(np.asarray(c[k])).to(DEV) for k in ("rnd", "pad", "perm") if c[k] is not None}
        cc, ff, ll = ip.crop_pc(coord, cd[:, 3:6], cd[:, 6], "train", voxel, voxel_max, variable=False, init_idx=c["init_idx"], **kw)
        pos.append(cc), col.append(ff), ys.append(ll)
    p, x, h = aug(torch.stack(pos), torch.stack(col), draws=t)
    return {"pos": p, "x": x, "heights": h, "y": torch.stack(ys)}


def _gpu(cdata, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(cdata)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _both(rooms_np, voxel_max, seed=3, voxel=VOXEL, dtype=None, same_draws=()):
    """the batched call and the per-room route on the same draws -> (batched, per-room, crop draws); same_draws: pairs (i, j)
    of rooms that get the same draws"""
    from amcontrast3d_amd import input_pipeline as ip
    rng = np.random.default_rng(seed)
    crop = [_crop_draws(rng, r, voxel_max, voxel) for r in rooms_np]
    t = {k: v[:len(rooms_np)].clone() for k, v in _transform_draws(np.random.default_rng(seed + 1000), 4, voxel_max).items()}
    for i, j in same_draws:
        crop[j] = crop[i]
        for k in t:
            t[k][j] = t[k][i]
    rooms = [_gpu(r, dtype) for r in rooms_np]
    aug = _aug()
    got = ip.s3dis_train_batch(rooms, aug, voxel, voxel_max, draws=_all_draws(crop, t))
    want = _per_room(rooms, aug, voxel_max, crop, t, voxel)
    assert got["pos"].shape == (len(rooms), voxel_max, 3) and got["heights"].shape == (len(rooms), voxel_max, 1)
    assert got["pos"].dtype == got["x"].dtype == got["heights"].dtype == torch.float32 and got["y"].dtype == torch.int64
    for k in KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    return got, want, crop


def _fixture(tag):
    g = load_golden("s3dis_input")
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_rooms_match_the_restatement_of_the_reference_run(tag):
    from amcontrast3d_amd import input_pipeline as ip
    c = _fixture(tag)
    vm = int(c["voxel_max"])
    cropped = len(c["count"]) >= vm
    r = {k: c[k] for k in ("rnd", "pad", "perm", "blend", "scale_u", "theta", "noise")}
    r["init_idx"] = int(c["init_idx"])
    r["contrast"], r["drop"] = bool(c["contrast_u"] < 0.2), bool(c["drop_u"] < 0.2)
    want = ref.train_item(c["cdata"], r, voxel_max=vm)  # pinned to the fixture's tensors by tests/test_s3dis_input_oracle.py
    d = {"contrast": np.array([r["contrast"]]), "blend": np.array([r["blend"]], dtype=np.float32), "scale_u": c["scale_u"][None],
         "theta": c["theta"][None], "noise": c["noise"][None], "drop": np.array([r["drop"]]),
         "rnd": [c["rnd"]], "init_idx": [r["init_idx"] if cropped else None], "pad": [None if cropped else c["pad"]],
         "perm": [c["perm"]]}
    out = ip.s3dis_train_batch([_gpu(c["cdata"])], _aug(), VOXEL, vm, draws=d)
    got = {k: out[k][0].cpu().numpy() for k in KEYS}
    np.testing.assert_array_equal(got["y"], want["y"])
    np.testing.assert_array_equal(got["heights"], want["heights"])
    np.testing.assert_array_equal(got["heights"], want["pos0"][:, 2:3])  # the cropped cloud's z before the transforms
    err = np.abs(got["pos"] - want["pos"]).max(), np.abs(got["x"] - want["x"]).max()
    print(tag, "max |pos - restatement|", err[0], "max |x - restatement|", err[1])
    np.testing.assert_allclose(got["pos"], want["pos"], rtol=0, atol=3e-6)
    np.testing.assert_allclose(got["x"], want["x"], rtol=0, atol=3e-5)
    # where the reference's unstable sorts chose as the stable ones do, the fixture's own tensors are compared
    if np.array_equal(want["idx_unique"], c["idx_unique"]) and (not cropped or np.array_equal(want["crop_idx"], c["crop_idx"])):
        np.testing.assert_array_equal(got["y"], c["y"])
        np.testing.assert_array_equal(got["heights"], c["heights"])
        np.testing.assert_allclose(got["pos"], c["pos"], rtol=0, atol=3e-6)
        np.testing.assert_allclose(got["x"], c["x"], rtol=0, atol=3e-5)


@pytest.fixture(scope="module")
def ragged():
    return [_room(1, 4500), _room(2, 6001), _room(3, 2999)]


def test_ragged_batch_with_a_cropped_and_a_padded_room(ragged):
    nv = sorted(len(_counts(r)) for r in ragged)
    vm = (nv[0] + nv[1]) // 2  # between two rooms' voxel counts: room 2 is padded, rooms 0 and 1 are cropped
    assert nv[0] < vm < nv[1] and all(len(r) % 64 for r in ragged)
    _, _, crop = _both(ragged, vm)
    assert sum(c["pad"] is not None for c in crop) == 1 and sum(c["init_idx"] is not None for c in crop) == 2


def test_the_same_room_twice_in_a_row(ragged):
    """equal keys meet at a segment boundary: the boundary must still start a voxel"""
    vm = len(_counts(ragged[0])) - 200
    got, _, _ = _both([ragged[2], ragged[0], ragged[0]], vm, same_draws=[(1, 2)])
    single, _, _ = _both([ragged[2], ragged[0]], vm)  # the same seed: the same draws for rooms 0 and 1
    for k in KEYS:
        assert torch.equal(got[k][1], got[k][2]) and torch.equal(got[k][1], single[k][1]), k


def test_lattice_room_where_crop_distances_tie():
    voxel = 0.03125  # exact in float32: lattice sites i * voxel stay exact, so symmetric sites are exactly equidistant
    rng = np.random.default_rng(5)
    ijk = np.stack(np.meshgrid(np.arange(24), np.arange(20), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    xyz = np.concatenate([ijk * voxel, ijk * voxel + voxel / 4], 0) + np.array([4.0, 8.0, 1.0])  # two points per voxel
    n = len(xyz)
    room = np.concatenate([xyz, rng.integers(0, 256, (n, 3)).astype(np.float64), rng.integers(0, 13, (n, 1)).astype(np.float64)], 1)
    room = room[rng.permutation(n)]
    count = _counts(room, voxel)
    assert len(count) == 24 * 20 * 3 and count.max() == 2
    vm = 700
    _, _, crop = _both([room, _room(6, 3001)], vm, voxel=voxel)
    item = ref.crop_item(room, crop[0], voxel, vm)
    assert len(np.unique(item["d2"])) < len(item["d2"]) // 2  # most distances are shared: the stable order decides the crop
    edge = item["d2"][item["crop_idx"][-1]]
    assert np.sum(item["d2"] == edge) > np.sum(item["d2"][item["crop_idx"]] == edge)  # and the cut falls inside a tie


def test_exactly_voxel_max_voxels_and_a_single_room(ragged):
    vm = len(_counts(ragged[0]))
    _, _, crop = _both([ragged[0]], vm)  # B = 1, N == voxel_max: a crop that keeps everything, in distance order
    assert crop[0]["init_idx"] is not None and crop[0]["pad"] is None
    _both([ragged[2], ragged[0]], vm)


def test_float64_and_float32_raw_input_of_the_same_values(ragged):
    rooms32 = [r.astype(np.float32) for r in ragged[:2]]
    vm = 3000  # between the two rooms' voxel counts
    a, _, _ = _both(rooms32, vm, dtype=torch.float32)
    b, _, _ = _both([r.astype(np.float64) for r in rooms32], vm, dtype=torch.float64)
    c, _, _ = _both(ragged[:2], vm)  # float64 values that the float32 cast rounds
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def _big_room(seed, n=300000):
    """300 k raw points: three jittered copies of a 10 m x 8 m relief, ~40 k occupied 4 cm voxels"""
    rng = np.random.default_rng(seed)
    nb = n // 3
    g = np.stack([rng.uniform(0, 10, nb), rng.uniform(0, 8, nb)], 1)
    z = 0.4 * np.sin(g[:, 0]) * np.cos(0.7 * g[:, 1]) + rng.choice([0.0, 1.5], nb)
    base = np.concatenate([g, z[:, None]], 1) + np.array([-30.0, 12.0, 0.4])
    xyz = np.concatenate([base + rng.uniform(-0.01, 0.01, base.shape) for _ in range(3)], 0)
    return np.concatenate([xyz, rng.integers(0, 256, (n, 3)).astype(np.float64), rng.integers(0, 13, (n, 1)).astype(np.float64)],
                          1)[rng.permutation(n)]


def test_two_rooms_of_300k_points_at_the_config_size():
    rooms = [_big_room(11), _big_room(12)]
    assert all(len(_counts(r)) >= 24000 for r in rooms)
    got, _, _ = _both(rooms, 24000)
    assert got["pos"].shape == (2, 24000, 3)


def test_generator_runs_are_reproducible_and_rooms_stay_apart():
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu(_room(20 + b, n, label=b)) for b, n in enumerate((4500, 2999, 6001))]
    aug = _aug()
    vm = 2400  # room 1 is padded, rooms 0 and 2 are cropped
    runs = [ip.s3dis_train_batch(rooms, aug, VOXEL, vm, generator=torch.Generator(device=DEV).manual_seed(7)) for _ in range(2)]
    for k in KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), k
    other = ip.s3dis_train_batch(rooms, aug, VOXEL, vm, generator=torch.Generator(device=DEV).manual_seed(8))
    assert not torch.equal(runs[0]["pos"], other["pos"])
    out = runs[0]
    assert out["pos"].shape == (3, vm, 3) and bool(torch.isfinite(out["pos"]).all()) and bool(torch.isfinite(out["x"]).all())
    # heights is the cropped cloud's gravity column before the transforms: every cloud sits at its own min corner
    assert torch.equal(out["heights"].amin(dim=(1, 2)), torch.zeros(3, device=DEV))
    for b in range(3):  # every label is a label of its own room
        assert bool((out["y"][b] == b).all())


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


def test_one_read_back_per_batch_on_the_generator_path():
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu(_room(30 + b, n)) for b, n in enumerate((4500, 2999, 6001))]
    aug = _aug()
    gen = torch.Generator(device=DEV).manual_seed(1)
    cd = rooms[0].float()
    coord = cd[:, :3] - cd[:, :3].min(0).values
    per_room = lambda: ip.crop_pc(coord, cd[:, 3:6], cd[:, 6], "train", VOXEL, 2400, variable=False, generator=gen)  # noqa: E731
    batched = lambda: ip.s3dis_train_batch(rooms, aug, VOXEL, 2400, generator=gen)  # noqa: E731
    per_room(), batched()  # warm: constants uploaded, code objects loaded
    n_room = len(_sync_warnings(per_room))
    if n_room < 1:
        pytest.skip("this build raises no synchronisation warning for crop_pc's read-backs")
    got = _sync_warnings(batched)
    print("synchronisation warnings: crop_pc of one room", n_room, "- s3dis_train_batch of three rooms", len(got))
    assert len(got) <= 1, [str(w.message) for w in got]


def test_errors():
    from amcontrast3d_amd import input_pipeline as ip
    aug = _aug()
    room_np = _room(40, 2999)
    room = _gpu(room_np)
    N = len(_counts(room_np))
    gen = torch.Generator(device=DEV).manual_seed(0)
    bad = lambda rooms, vm=1500, **kw: ip.s3dis_train_batch(rooms, aug, VOXEL, vm, generator=gen, **kw)  # noqa: E731
    with pytest.raises(ValueError):
        bad([])
    for malformed in (room[:, :6], room.cpu(), room.long(), room[:0], room.reshape(-1)):
        with pytest.raises(ValueError):
            bad([room, malformed])
    with pytest.raises(ValueError):
        bad([room], vm=None)
    ok = _crop_draws(np.random.default_rng(0), room_np, N - 100)
    for key, value in (("rnd", ok["rnd"][:-1]), ("rnd", -1 - ok["rnd"]), ("init_idx", N), ("init_idx", -1),
                       ("perm", ok["perm"][:-1]), ("perm", np.zeros_like(ok["perm"]))):
        with pytest.raises(ValueError):
            bad([room], vm=N - 100, draws={key: [torch.from_numpy(value) if isinstance(value, np.ndarray) else value]})
    for value in (np.zeros(99, dtype=np.int64), np.full(100, N, dtype=np.int64)):  # N + 100 slots: 100 padding draws below N
        with pytest.raises(ValueError):
            bad([room], vm=N + 100, draws={"pad": [torch.from_numpy(value)]})
    with pytest.raises(ValueError):
        bad([room], draws={"rnd": [None, None]})
    with pytest.raises(ValueError):
        bad([room], draws={"scale_u": torch.zeros(2, 3)})
    with pytest.raises(ValueError):  # the collate stacks: rooms that stay at their own sizes cannot form one batch
        bad([room, _gpu(_room(41, 4500))], vm=100000, variable=True)
    out = bad([room], vm=100000, variable=True)  # one room at its own size is fine
    assert out["pos"].shape == (1, N, 3)


def _feed(labels=(0, 1, 2), **kw):
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu(_room(50 + b, 2999 + 500 * b, label=b)) for b in labels]
    return ip.S3DISTrainFeed(rooms, _aug(), **kw)


def test_feed_epochs():
    feed = _feed(batch_size=2, loop=2, voxel_max=2048, generator=torch.Generator(device=DEV).manual_seed(2))
    assert len(feed) == 3
    orders = []
    for _ in range(3):
        batches = list(feed)
        assert len(batches) == 3 and all(b["pos"].shape == (2, 2048, 3) and b["y"].shape == (2, 2048) for b in batches)
        ids = [int(b["y"][i, 0]) for b in batches for i in range(2)]
        for b in batches:  # a cloud's labels are its room's
            assert bool((b["y"] == b["y"][:, :1]).all())
        assert sorted(ids) == [0, 0, 1, 1, 2, 2]  # each room exactly `loop` times
        orders.append((ids, batches[0]["pos"]))
    # further epochs from the same generator: other draws and another order of the rooms (three epochs agree once in 8100)
    assert not torch.equal(orders[0][1], orders[1][1])
    assert len({tuple(ids) for ids, _ in orders}) > 1, orders
    again = _feed(batch_size=2, loop=2, voxel_max=2048, generator=torch.Generator(device=DEV).manual_seed(2))
    assert [int(b["y"][i, 0]) for b in again for i in range(2)] == orders[0][0]  # the same seed: the same epoch


def test_two_training_iterations_on_feed_batches():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    import openpoints.utils as ou
    from amcontrast3d_amd import configs, train
    from openpoints.loss import build_criterion_from_cfg
    from openpoints.models import build_model_from_cfg
    from openpoints.utils import EasyConfig
    torch.manual_seed(0)
    c = EasyConfig(); c.update(configs.model_cfg("S", dropout=0, width=16))
    model = build_model_from_cfg(c).to(DEV)
    cc = EasyConfig(); cc.update(configs.criterion_cfg())
    crit = build_criterion_from_cfg(cc).to(DEV)
    cfg = EasyConfig()
    cfg.update({"num_classes": 13, "ignore_index": None, "ambiguity_args": configs.ambiguity_args("s3dis"),
                "feature_keys": "x,heights", "use_amp": False, "step_per_update": 1, "grad_norm_clip": 10, "sched_on_epoch": True})
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    from amcontrast3d_amd import input_pipeline as ip
    rooms = [_gpu(_room(60 + b, 6001 + 1500 * b)) for b in range(4)]
    feed = ip.S3DISTrainFeed(rooms, _aug(), batch_size=2, voxel_max=4096, generator=torch.Generator(device=DEV).manual_seed(5))
    assert len(feed) == 2
    made = []
    real = ou.ConfusionMatrix

    class Recording(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    ou.ConfusionMatrix = Recording
    try:
        got = train.train_one_epoch(model, feed, crit, opt, None, None, 1, cfg)
    finally:
        ou.ConfusionMatrix = real
    assert np.isfinite(got[0])
    assert len(made) == 1 and int(made[0].value.sum()) == 2 * 2 * 4096
