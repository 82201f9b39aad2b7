"""ScanNet's training input on the device (csrc/scannet_input.hip, the *_f64 kernels of csrc/voxel.hip,
augment.ScanNetTrainAugment, input_pipeline.scannet_train_batch): against what the reference's own ScanNet.__getitem__
returned for the same raw rooms and draws (tests/golden/scannet_input.npz), and against the numpy restatement
(tests/scannet_input_ref.py) at full size and on edge cases.  Every specified quantity is compared exactly; numpy's argsort
is unstable, so where the reference leaves an order unspecified (points inside one voxel, equidistant crop points) the
comparison is by voxel / as sets, as in tests/test_gpu_input.py."""
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


def _aug():
    from amcontrast3d_amd.augment import ScanNetTrainAugment
    return ScanNetTrainAugment(**KWARGS)


def _case(tag):
    g = load_golden("scannet_input")
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/")}


def _draws(rooms_draws, with_R=True):
    """per-room draw dicts (numpy) -> the `draws` argument of scannet_train_batch"""
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


def _transform(aug, room, d):
    coord, feat, _ = room
    off = torch.tensor([0, coord.shape[0]], dtype=torch.int64, device=DEV)
    return aug(coord, feat, off, draws=d)


def _want(coord, feat, label, r, voxel_max, variable=False, R=None):
    pos, x = ref.transform_room(coord, feat, r["R"] if R is None else R, r["scale"], r["mirror_u"], r["contrast_u"],
                                r["blend"], r["drop_u"])
    return pos, x, ref.crop_room(pos, x, label, VOXEL, voxel_max, variable, r["rnd"], r.get("init_idx"), r.get("pad"), r["perm"])


def _assert_batch(out, wants):
    for b, w in enumerate(wants):
        np.testing.assert_array_equal(out["pos"][b].cpu().numpy(), w["pos"])
        np.testing.assert_array_equal(out["x"][b].cpu().numpy(), w["x"])
        np.testing.assert_array_equal(out["y"][b].cpu().numpy(), w["y"])
        np.testing.assert_array_equal(out["heights"][b].cpu().numpy(), w["heights"])
    assert out["pos"].dtype == out["x"].dtype == out["heights"].dtype == torch.float32 and out["y"].dtype == torch.int64


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_rooms_match_the_reference_run(tag):
    from amcontrast3d_amd import input_pipeline as ip
    c = _case(tag)
    aug = _aug()
    room = _gpu_room(c["coord"], c["feat"], c["label"])
    r = _fixture_draws(c)
    d = _draws([r])
    pos, x, stats = _transform(aug, room, d)
    np.testing.assert_array_equal(pos.cpu().numpy(), c["t_pos"])     # float64 positions, bit for bit (OpenBLAS's FMA order)
    np.testing.assert_array_equal(x.cpu().numpy(), c["t_x"])         # colours after contrast / drop / normalise
    p = pos - pos.min(0).values
    key, idx_sort, voxel_idx, start, count = ip._voxel_tables(p, VOXEL)
    np.testing.assert_array_equal(key.cpu().numpy().view(np.uint64), c["key"])
    np.testing.assert_array_equal(count.cpu().numpy(), c["count"])
    pick = ip.voxelize(p, VOXEL, rnd=torch.from_numpy(c["rnd"])).cpu().numpy()
    np.testing.assert_array_equal(c["key"][pick], c["key"][c["idx_unique"]])  # the voxel of every mode-0 pick
    vm = int(c["voxel_max"])
    if r["init_idx"] is not None:  # the crop of the reference's voxelised cloud
        d2, ci = ip.crop_nearest(p[torch.from_numpy(c["idx_unique"]).to(DEV)], r["init_idx"], vm)
        assert d2.dtype == torch.float64
        np.testing.assert_array_equal(d2.cpu().numpy(), c["d2"])
        ci = ci.cpu().numpy()
        np.testing.assert_array_equal(c["d2"][ci], c["d2"][c["crop_idx"]])
        assert set(ci.tolist()) == set(c["crop_idx"].tolist()) or np.sum(c["d2"] == c["d2"][c["crop_idx"][-1]]) > 1
    out = ip.scannet_train_batch([room], aug, VOXEL, vm, variable=False, draws=d)
    _, _, want = _want(c["coord"], c["feat"], c["label"], r, vm)
    _assert_batch(out, [want])
    # the final tensors follow the picks: where the reference's unstable sorts chose other points of the same voxels, the
    # restatement (pinned to the fixture's final tensors on the reference's own picks by test_scannet_input_oracle.py)
    # stands in for it; where they chose alike, the fixture itself is compared
    if np.array_equal(want["idx_unique"], c["idx_unique"]) and (r["init_idx"] is None or np.array_equal(want["crop_idx"], c["crop_idx"])):
        for k in ("pos", "x", "y", "heights"):
            np.testing.assert_array_equal(out[k][0].cpu().numpy(), c[k])


def test_crop_pc_on_float64_rooms_with_passed_draws():
    """crop_pc itself on a transformed (float64) room, with the fixture's draws (case b: the variable=False padding's
    np.random.choice draw passed as `pad`), gives what scannet_train_batch gives"""
    from amcontrast3d_amd import input_pipeline as ip
    for tag in ("a", "b"):
        c = _case(tag)
        room = _gpu_room(c["coord"], c["feat"], c["label"])
        aug = _aug()
        d = _draws([_fixture_draws(c)])
        pos, x, _ = _transform(aug, room, d)
        kw = {"init_idx": int(c["init_idx"])} if c["init_idx"] >= 0 else {"pad": torch.from_numpy(c["pad"])}
        cc, ff, ll = ip.crop_pc(pos, x, room[2], "train", VOXEL, int(c["voxel_max"]), variable=False,
                                rnd=torch.from_numpy(c["rnd"]), perm=torch.from_numpy(c["perm"]).to(DEV), **kw)
        out = ip.scannet_train_batch([room], aug, VOXEL, int(c["voxel_max"]), draws=d)
        assert cc.dtype == torch.float32
        assert torch.equal(cc, out["pos"][0]) and torch.equal(ff, out["x"][0]) and torch.equal(ll, out["y"][0])


def test_default_rotation_gives_the_reference_voxels_and_crop():
    from amcontrast3d_amd import input_pipeline as ip
    for tag in ("a", "b"):
        c = _case(tag)
        room = _gpu_room(c["coord"], c["feat"], c["label"])
        pos, _, _ = _transform(_aug(), room, _draws([_fixture_draws(c)], with_R=False))  # cos / sin on the host
        p = pos - pos.min(0).values
        key = ip._voxel_tables(p, VOXEL)[0]
        np.testing.assert_array_equal(key.cpu().numpy().view(np.uint64), c["key"])
        if c["init_idx"] >= 0:
            d2, ci = ip.crop_nearest(p[torch.from_numpy(c["idx_unique"]).to(DEV)], int(c["init_idx"]), int(c["voxel_max"]))
            assert set(ci.cpu().tolist()) == set(c["crop_idx"].tolist())


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


def _room_draws(rng, coord, feat, label, voxel_max, contrast=None, drop=None, variable=False):
    """draws for one room with the restatement's voxel count (rnd / init / pad / perm need it)"""
    import math
    r = {"angle": float(rng.uniform(-math.pi, math.pi)), "scale": float(rng.uniform(0.8, 1.2)), "mirror_u": rng.random(3),
         "contrast_u": float(rng.random()) if contrast is None else (0.1 if contrast else 0.9), "blend": float(rng.random()),
         "drop_u": float(rng.random()) if drop is None else (0.1 if drop else 0.9)}
    r["R"] = ref.rotation(r["angle"])
    pos, _ = ref.transform_room(coord, feat, r["R"], r["scale"], r["mirror_u"], r["contrast_u"], r["blend"], r["drop_u"])
    p = pos - pos.min(0)
    key = ref.fnv_hash_vec(np.floor(p / np.array(VOXEL)))
    count = np.unique(key, return_counts=True)[1]
    N = len(count)
    r["rnd"] = rng.integers(0, count.max(), N)
    r["init_idx"] = int(rng.integers(N)) if N >= voxel_max else None
    r["pad"] = rng.integers(0, N, voxel_max - N) if (N < voxel_max and not variable) else None
    r["perm"] = rng.permutation(voxel_max if (N >= voxel_max or not variable) else N)
    return r, N


def test_full_size_batch_against_the_restatement_and_deterministic():
    from amcontrast3d_amd import input_pipeline as ip
    rng = np.random.default_rng(7)
    rooms = [_big_room(1), _big_room(2)]
    draws, wants = [], []
    for i, (coord, feat, label) in enumerate(rooms):
        r, N = _room_draws(rng, coord, feat, label, 64000, contrast=(i == 0), drop=False)
        assert N >= 64000 and len(coord) > 140000
        draws.append(r)
        wants.append(_want(coord, feat, label, r, 64000)[2])
    g = [_gpu_room(*rm) for rm in rooms]
    aug = _aug()
    out = ip.scannet_train_batch(g, aug, VOXEL, 64000, draws=_draws(draws))
    assert out["pos"].shape == (2, 64000, 3) and out["heights"].shape == (2, 64000, 1) and out["y"].shape == (2, 64000)
    _assert_batch(out, wants)
    # the device's own draws: two runs from the same seed are bit-identical
    runs = [ip.scannet_train_batch(g, aug, VOXEL, 64000, generator=torch.Generator(device=DEV).manual_seed(3)) for _ in range(2)]
    for k in ("pos", "x", "heights", "y"):
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert runs[0]["pos"].shape == (2, 64000, 3) and float(runs[0]["pos"].min()) == 0.0


def _small_room(seed, n_base=3000, copies=3):
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(0, 2.0, n_base), rng.uniform(0, 1.5, n_base), rng.choice([0.0, 1.2], n_base) + rng.uniform(0, 0.3, n_base)], 1)
    coord = np.concatenate([base + rng.uniform(-0.008, 0.008, base.shape) for _ in range(copies)], 0).astype(np.float32)
    feat = rng.uniform(-1, 1, coord.shape).astype(np.float32)
    label = rng.integers(-1, 20, len(coord)).astype(np.int64)
    label[label < 0] = -100
    return coord, feat, label


def _run_edge(rooms, voxel_max, variable=False, **kw):
    from amcontrast3d_amd import input_pipeline as ip
    rng = np.random.default_rng(11)
    draws, wants = [], []
    for coord, feat, label in rooms:
        r, _ = _room_draws(rng, coord, feat, label, voxel_max(coord, feat, label) if callable(voxel_max) else voxel_max,
                           variable=variable, **kw)
        draws.append(r)
    vm = voxel_max(*rooms[0]) if callable(voxel_max) else voxel_max
    for (coord, feat, label), r in zip(rooms, draws):
        wants.append(_want(coord, feat, label, r, vm, variable))
    out = ip.scannet_train_batch([_gpu_room(*rm) for rm in rooms], _aug(), VOXEL, vm, variable=variable, draws=_draws(draws))
    _assert_batch(out, [w[2] for w in wants])
    return out, wants


def test_edge_constant_colour_channel_with_contrast_gives_numpys_nan():
    coord, feat, label = _small_room(3)
    feat[:, 1] = 0.25  # hi == lo: 255 / 0 = inf, 0 * inf = NaN, max() = NaN, NaN > 1 is false: no /255
    out, wants = _run_edge([(coord, feat, label)], 4000, contrast=True, drop=False)
    x = out["x"][0].cpu().numpy()
    assert np.all(np.isnan(x[:, 1])) and not np.any(np.isnan(x[:, [0, 2]]))
    assert np.isnan(wants[0][1].max())


def test_edge_colours_already_at_most_one():
    coord, feat, label = _small_room(4)
    feat = np.float32(-1) + np.abs(feat) * np.float32(0.007)  # (feat + 1) * 127.5 <= 1: no /255
    out, wants = _run_edge([(coord, feat, label)], 4000, contrast=False, drop=False)
    assert wants[0][1].max() <= (1 - ref.COLOR_MEAN[0]) / ref.COLOR_STD[0] + 1e-6


def test_edge_exactly_voxel_max_voxels():
    def nvox(coord, feat, label):  # the room's own voxel count (a deterministic function of the draws below)
        r, n = _room_draws(np.random.default_rng(11), coord, feat, label, 1)
        return n
    out, wants = _run_edge([_small_room(5)], nvox)
    assert "crop_idx" in wants[0][2] and len(wants[0][2]["crop_idx"]) == out["pos"].shape[1]


def test_edge_variable_rooms():
    from amcontrast3d_amd import input_pipeline as ip
    out, wants = _run_edge([_small_room(6)], 100000, variable=True)  # no crop, no padding: the room's own voxel count
    assert out["pos"].shape[1] == len(wants[0][2]["idx_unique"]) < 100000
    with pytest.raises(ValueError):  # the collate stacks: rooms of different sizes cannot form one batch
        ip.scannet_train_batch([_gpu_room(*_small_room(6)), _gpu_room(*_small_room(7, n_base=2000))], _aug(), VOXEL, 100000,
                               variable=True, generator=torch.Generator(device=DEV).manual_seed(0))


def test_fp32_voxelize_and_crop_unchanged():
    from amcontrast3d_amd import input_pipeline as ip
    from oracle import input_ref
    coord, _, _ = _small_room(8)
    coord = (coord - coord.min(0)).astype(np.float32)
    g = torch.from_numpy(coord).to(DEV)
    key, idx_sort, voxel_idx, start, count = ip._voxel_tables(g, 0.04)
    want = input_ref.voxelize(coord, 0.04, mode=1)
    np.testing.assert_array_equal(idx_sort.cpu().numpy(), want[0])
    np.testing.assert_array_equal(voxel_idx.cpu().numpy(), want[1])
    np.testing.assert_array_equal(count.cpu().numpy(), want[2])
    key64 = ip._voxel_tables(g.double(), 0.04)[0]  # the f64 kernel on the same values: the same cells
    assert torch.equal(key, key64)
    d2, ci = ip.crop_nearest(g, 17, 2000)
    assert d2.dtype == torch.float32 and ci.dtype == torch.int64
    wd2, wci = input_ref.crop_nearest(coord, 17, 2000)
    np.testing.assert_array_equal(d2.cpu().numpy(), wd2)
    np.testing.assert_array_equal(ci.cpu().numpy(), wci)


def test_two_training_iterations_on_scannet_batches():
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
    gen = torch.Generator(device=DEV).manual_seed(5)
    aug = _aug()
    batches = [ip.scannet_train_batch([_gpu_room(*_small_room(20 + 2 * i)), _gpu_room(*_small_room(21 + 2 * i))], aug, VOXEL,
                                      4096, generator=gen) for i in range(2)]
    counted = sum(int((b["y"] != -100).sum()) for b in batches)
    made = []
    real = ou.ConfusionMatrix

    class Recording(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    ou.ConfusionMatrix = Recording
    try:
        got = train.train_one_epoch(model, [dict(b) for b in batches], crit, opt, None, None, 1, cfg)
    finally:
        ou.ConfusionMatrix = real
    assert np.isfinite(got[0])
    assert len(made) == 1 and int(made[0].value.sum()) == counted
