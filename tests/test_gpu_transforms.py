"""amcontrast3d_amd.transforms.TransformChain on the device (csrc/transforms.hip) against what the reference's own classes
recorded (tests/golden/transforms.npz), with the recorded draws: every class alone and four whole chains, as one ragged batch
of the five cloud sizes and as a dense 3 x 777 batch.  Exact where every op is elementwise or min / max based (the float64
np.dot rotations included); within test_gpu_augment.py's bands where the chain holds a mean or the float32 pos @ rot.T."""
import numpy as np
import pytest
import torch

import transforms_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = load_golden("transforms")
CASES = sorted(G["meta"]["cases"])
S3DIS = ["ChromaticAutoContrast", "PointsToTensor", "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation", "PointCloudJitter",
         "ChromaticDropGPU", "ChromaticNormalize"]  # cfgs/s3dis/default.yaml
S3DIS_KW = {"color_drop": 0.2, "gravity_dim": 2, "scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02}
SCANNET = ["RandomRotateZ", "RandomScale", "ChromaticAutoContrast", "RandomDropFeature", "NumpyChromaticNormalize"]
SCANNET_KW = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
              "color_mean": [0.46259782, 0.46253258, 0.46253258], "color_std": [0.693565, 0.6852543, 0.68061745]}


def _chain(case):
    from amcontrast3d_amd.transforms import TransformChain
    meta = G["meta"]["cases"][case]
    return TransformChain(meta["names"], meta["kwargs"]), meta["names"]


def _batch_draws(chain, per_cloud):
    """per-cloud recorded draws -> the batch's: cloud draws stacked, point draws concatenated, given rotations stacked"""
    out = {}
    keys = list(chain.spec()) + sorted({k for d in per_cloud for k in d if k.endswith(".R")})
    for key in keys:
        vals = [np.asarray(d[key]) for d in per_cloud]
        if key.endswith(".R"):
            out[key] = torch.from_numpy(np.stack(vals))
        elif chain.spec()[key][0] == "cloud":
            out[key] = torch.from_numpy(np.stack([v.reshape(-1) for v in vals])).reshape(
                (len(vals),) + ((chain.spec()[key][1],) if chain.spec()[key][1] else ()))
        else:
            out[key] = torch.from_numpy(np.concatenate(vals))
    return out


def _np(out, lo, hi):
    return {k: out[k][lo:hi].cpu().numpy() for k in ("pos", "x", "heights")}


@pytest.mark.parametrize("case", CASES)
def test_ragged_batch_of_the_five_clouds_matches_the_reference_run(case):
    chain, names = _chain(case)
    sizes = G["meta"]["sizes"]
    clouds = range(len(sizes))
    pos = torch.from_numpy(np.concatenate([ref.cloud_inputs(G, c)[0] for c in clouds])).to(DEV)
    x = torch.from_numpy(np.concatenate([ref.cloud_inputs(G, c)[1] for c in clouds])).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
    out = chain({"pos": pos, "x": x, "offsets": off}, draws=_batch_draws(chain, [ref.cloud_draws(G, case, c) for c in clouds]))
    assert out["pos"].shape == (sum(sizes), 3) and out["x"].shape == (sum(sizes), 3) and out["heights"].shape == (sum(sizes), 1)
    for c in clouds:
        ref.compare(_np(out, int(off[c]), int(off[c + 1])), ref.expected(G, case, c), names, f"{case} cloud {c}")


@pytest.mark.parametrize("case", CASES)
def test_dense_batch_matches_the_reference_run(case):
    chain, names = _chain(case)
    p, x = ref.cloud_inputs(G, 4)
    pos = torch.from_numpy(np.stack([p] * 3)).to(DEV)
    col = torch.from_numpy(np.stack([x] * 3)).to(DEV)
    out = chain({"pos": pos, "x": col}, draws=_batch_draws(chain, [ref.cloud_draws(G, case, 4)] * 3))
    assert out["pos"].shape == (3, 777, 3) and out["heights"].shape == (3, 777, 1)
    want = ref.expected(G, case, 4)
    for b in range(3):
        ref.compare({k: out[k][b].cpu().numpy() for k in ("pos", "x", "heights")}, want, names, f"{case} dense {b}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_s3dis_default_chain_from_the_yaml_list_matches_the_s3dis_fixture(tag):
    from amcontrast3d_amd.transforms import build_transforms_from_cfg
    g = load_golden("augment_s3dis")
    # the fixture's two runs were recorded with their own gate probabilities
    kwargs = dict(g["meta"], p=float(g[f"{tag}/p_contrast"]), color_drop=float(g[f"{tag}/p_drop"]))
    chain = build_transforms_from_cfg("train", {"train": S3DIS, "kwargs": kwargs})
    d = {"0.u": torch.tensor([float(g[f"{tag}/contrast_u"])], dtype=torch.float64),
         "0.blend": torch.tensor([float(g[f"{tag}/blend"]) if f"{tag}/blend" in g else 0.0], dtype=torch.float64),
         "2.scale_u": torch.from_numpy(g[f"{tag}/scale_u"]).reshape(1, 3), "4.theta": torch.from_numpy(g[f"{tag}/theta"]).reshape(1, 3),
         "4.order": torch.tensor([[0, 1, 2]]), "5.noise": torch.from_numpy(g[f"{tag}/noise"]),
         "6.u": torch.from_numpy(g[f"{tag}/drop_u"]).reshape(1)}
    out = chain({"pos": torch.from_numpy(g["coord"]).unsqueeze(0).to(DEV), "x": torch.from_numpy(g["feat"]).unsqueeze(0).to(DEV)}, draws=d)
    np.testing.assert_allclose(out["pos"][0].cpu().numpy(), g[f"{tag}/pos"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(out["x"][0].cpu().numpy(), g[f"{tag}/x"], rtol=0, atol=2e-5)
    np.testing.assert_array_equal(out["heights"][0].cpu().numpy(), g[f"{tag}/heights"])


def test_same_draws_same_bits_and_fresh_draws_differ():
    chain, _ = _chain("chain_center_flip")
    gen = torch.Generator(device=DEV).manual_seed(5)
    sizes = [1, 1024, 1025, 5000]
    rng = np.random.default_rng(0)
    pos = torch.from_numpy(rng.uniform(0, 6, (sum(sizes), 3)).astype(np.float32)).to(DEV)
    x = torch.from_numpy(np.round(rng.uniform(0, 255, (sum(sizes), 3))).astype(np.float32)).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
    data = {"pos": pos, "x": x, "offsets": off, "sizes": sizes}
    d = chain.draw(sizes, DEV, gen)
    assert all(v.is_cuda for v in d.values())
    a, b = chain(data, draws=d), chain(data, draws=d)
    assert bool(torch.isnan(a["pos"][0]).all())  # the one-point cloud: 0 / 0 in the normalisation, as in the reference
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a), "the same bits, NaNs included"
    up, _ = _chain("chain_upstream")
    p2 = torch.from_numpy(np.stack([rng.uniform(0, 6, (777, 3)).astype(np.float32)] * 2)).to(DEV)
    x2 = torch.from_numpy(np.stack([np.round(rng.uniform(0, 255, (777, 3))).astype(np.float32)] * 2)).to(DEV)
    o = up({"pos": p2, "x": x2}, generator=gen)
    assert o["pos"].dtype == torch.float64 and not torch.equal(o["pos"][0], o["pos"][1])  # the same cloud twice, its own draws each


def test_the_door_checks():
    chain, _ = _chain("chain_scannet")
    pos, x = torch.zeros(10, 3, device=DEV), torch.zeros(10, 3, device=DEV)
    off = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="empty"):
        chain({"pos": pos, "x": x, "offsets": off([0, 4, 4, 10])})
    with pytest.raises(ValueError, match="decrease"):
        chain({"pos": pos, "x": x, "offsets": off([0, 6, 4, 10])})
    with pytest.raises(ValueError, match="empty"):
        chain({"pos": pos, "x": x, "offsets": off([0, 10, 10]), "sizes": [10, 0]})
    d = chain.draw([4, 6], DEV)
    d["1.scale"] = d["1.scale"][:1]
    with pytest.raises(ValueError, match="1.scale"):
        chain({"pos": pos, "x": x, "offsets": off([0, 4, 10])}, draws=d)


def _s3dis_room(seed, n):
    rng = np.random.default_rng(seed)
    nb = -(-n // 3)
    base = np.stack([rng.uniform(0, 2.0, nb), rng.uniform(0, 1.5, nb), rng.choice([0.0, 1.2], nb) + 0.2 * rng.uniform(0, 1, nb)], 1) + np.array([21.5, -3.25, 0.7])
    xyz = np.concatenate([base + rng.uniform(-0.015, 0.015, base.shape) for _ in range(3)], 0)[:n]
    return np.concatenate([xyz, rng.integers(0, 256, (n, 3)).astype(np.float64), rng.integers(0, 13, (n, 1)).astype(np.float64)], 1)


def test_s3dis_train_batch_takes_a_chain_and_agrees_with_the_fixed_class():
    from amcontrast3d_amd import input_pipeline as ip
    from amcontrast3d_amd.augment import S3DISTrainAugment
    from amcontrast3d_amd.transforms import build_transforms_from_cfg
    rooms = [torch.from_numpy(_s3dis_room(s, 6000)).to(DEV) for s in (1, 2)]
    B, N = 2, 1500
    gen = torch.Generator(device=DEV).manual_seed(3)
    contrast, drop = torch.tensor([True, False], device=DEV), torch.tensor([False, True], device=DEV)
    blend, scale_u = torch.rand(B, device=DEV, generator=gen), torch.rand(B, 3, device=DEV, generator=gen)
    theta = torch.zeros(B, 3, dtype=torch.float64, device=DEV)
    theta[:, 2] = (torch.rand(B, dtype=torch.float64, device=DEV, generator=gen) * 2 - 1) * np.pi
    noise = torch.randn(B, N, 3, device=DEV, generator=gen)
    fixed = ip.s3dis_train_batch(rooms, S3DISTrainAugment(**S3DIS_KW), 0.04, N, generator=torch.Generator(device=DEV).manual_seed(7),
                                 draws={"contrast": contrast, "blend": blend, "scale_u": scale_u, "theta": theta, "noise": noise, "drop": drop})
    chain = build_transforms_from_cfg("train", {"train": S3DIS, "kwargs": S3DIS_KW})
    got = ip.s3dis_train_batch(rooms, chain, 0.04, N, generator=torch.Generator(device=DEV).manual_seed(7),
                               draws={"0.u": (~contrast).double(), "0.blend": blend.double(), "2.scale_u": scale_u, "4.theta": theta,
                                      "4.order": torch.tensor([[0, 1, 2]] * B, device=DEV), "5.noise": noise.reshape(B * N, 3),
                                      "6.u": (~drop).float()})
    assert got["pos"].shape == (B, N, 3) and got["x"].shape == (B, N, 3) and got["heights"].shape == (B, N, 1) and got["y"].shape == (B, N)
    assert got["pos"].dtype == got["x"].dtype == got["heights"].dtype == torch.float32 and got["y"].dtype == torch.int64
    np.testing.assert_allclose(got["pos"].cpu().numpy(), fixed["pos"].cpu().numpy(), rtol=0, atol=ref.POS_BAND)
    np.testing.assert_allclose(got["x"].cpu().numpy(), fixed["x"].cpu().numpy(), rtol=0, atol=ref.X_BAND)
    assert torch.equal(got["heights"], fixed["heights"]) and torch.equal(got["y"], fixed["y"])
    # a list that differs from the shipped one runs exactly the transforms it names: no rotation, no jitter
    plain = build_transforms_from_cfg("train", {"train": ["PointsToTensor", "PointCloudXYZAlign", "ChromaticNormalize"], "kwargs": S3DIS_KW})
    out = ip.s3dis_train_batch(rooms, plain, 0.04, N, generator=torch.Generator(device=DEV).manual_seed(7))
    assert float(out["pos"][..., 2].min()) == 0.0 and abs(float(out["pos"][0, :, 0].double().mean())) < 1e-5


def _scannet_room(seed, n_base=3000):
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(0, 2.0, n_base), rng.uniform(0, 1.5, n_base), rng.choice([0.0, 1.2], n_base) + rng.uniform(0, 0.3, n_base)], 1)
    coord = np.concatenate([base + rng.uniform(-0.008, 0.008, base.shape) for _ in range(3)], 0).astype(np.float32)
    return tuple(torch.from_numpy(a).to(DEV) for a in (coord, rng.uniform(-1, 1, coord.shape).astype(np.float32),
                                                        rng.integers(0, 20, len(coord)).astype(np.int64)))


def test_scannet_train_rooms_takes_a_chain_and_agrees_with_the_fixed_class():
    from amcontrast3d_amd import input_pipeline as ip
    from amcontrast3d_amd.augment import ScanNetTrainAugment
    from amcontrast3d_amd.transforms import build_transforms_from_cfg
    rooms = [_scannet_room(11), _scannet_room(12, 2500)]
    B, N = 2, 2000
    aug = ScanNetTrainAugment(**SCANNET_KW)
    d = aug.draw(B, torch.Generator().manual_seed(4))
    d["contrast_u"], d["drop_u"] = torch.tensor([0.1, 0.9], dtype=torch.float64), torch.tensor([0.9, 0.1], dtype=torch.float64)
    R = torch.stack([aug.rotation(float(a)) for a in d["angle"]])
    fixed = ip.scannet_train_rooms(rooms, aug, 0.02, N, generator=torch.Generator(device=DEV).manual_seed(7), draws=dict(d, R=R))
    chain = build_transforms_from_cfg("train", {"train": SCANNET, "kwargs": SCANNET_KW})
    got = ip.scannet_train_rooms(rooms, chain, 0.02, N, generator=torch.Generator(device=DEV).manual_seed(7),
                                 draws={"0.angle": d["angle"], "0.R": R, "1.scale": d["scale"].reshape(B, 1), "1.mirror_u": d["mirror_u"],
                                        "2.u": d["contrast_u"], "2.blend": d["blend"], "3.u": d["drop_u"]})
    assert got["pos"].shape == (B, N, 3) and got["x"].shape == (B, N, 3) and got["heights"].shape == (B, N, 1) and got["y"].shape == (B, N)
    assert got["pos"].dtype == got["x"].dtype == got["heights"].dtype == torch.float32 and got["y"].dtype == torch.int64
    np.testing.assert_allclose(got["pos"].cpu().numpy(), fixed["pos"].cpu().numpy(), rtol=0, atol=ref.POS_BAND)
    np.testing.assert_allclose(got["x"].cpu().numpy(), fixed["x"].cpu().numpy(), rtol=0, atol=ref.X_BAND)
    assert torch.equal(got["y"], fixed["y"])
    up = build_transforms_from_cfg("train", {"train": G["meta"]["cases"]["chain_upstream"]["names"], "kwargs": SCANNET_KW})
    out = ip.scannet_train_rooms(rooms, up, 0.02, N, generator=torch.Generator(device=DEV).manual_seed(7))
    assert out["pos"].shape == (B, N, 3) and out["pos"].dtype == torch.float32 and bool(torch.isfinite(out["x"]).all())
