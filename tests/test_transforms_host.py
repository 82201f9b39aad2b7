"""amcontrast3d_amd.transforms on the host: the builder, the compiled plans, and the numpy restatement (tests/transforms_ref.py)
against what the reference's own classes recorded (tests/golden/transforms.npz)."""
import numpy as np
import pytest

import transforms_ref as ref
from conftest import load_golden
from amcontrast3d_amd import transforms as T

G = load_golden("transforms")
CASES = sorted(G["meta"]["cases"])
S3DIS = ["ChromaticAutoContrast", "PointsToTensor", "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation", "PointCloudJitter",
         "ChromaticDropGPU", "ChromaticNormalize"]


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_recorded_reference_run(case):
    meta = G["meta"]["cases"][case]
    for c in range(len(G["meta"]["sizes"])):
        pos, x = ref.cloud_inputs(G, c)
        with np.errstate(all="ignore"):
            got = ref.run_chain(meta["names"], meta["kwargs"], pos, x, ref.cloud_draws(G, case, c))
        ref.compare(got, ref.expected(G, case, c), meta["names"], f"{case} cloud {c}")


def test_every_supported_class_is_recorded_alone_and_the_chains_whole():
    alone = {tuple(n for n in G["meta"]["cases"][c]["names"] if n != "PointsToTensor" or len(G["meta"]["cases"][c]["names"]) == 1)
             for c in CASES if not c.startswith("chain_")}
    assert {n for names in alone for n in names} == set(T.REGISTRY)
    assert {c for c in CASES if c.startswith("chain_")} == {"chain_s3dis", "chain_scannet", "chain_upstream", "chain_center_flip"}
    assert G["meta"]["sizes"] == [1, 63, 64, 65, 777]


def test_builder_returns_none_for_a_missing_or_empty_list():
    assert T.build_transforms_from_cfg("train", {"val": ["PointsToTensor"]}) is None
    assert T.build_transforms_from_cfg("train", {"train": []}) is None
    one = T.build_transforms_from_cfg("val", {"val": ["NumpyChromaticNormalize"]})
    assert isinstance(one, T.TransformChain) and one.names == ["NumpyChromaticNormalize"]


def test_builder_uses_the_reference_defaults():
    c = T.build_transforms_from_cfg("train", {"train": ["RandomRotateZ", "RandomScale", "ChromaticAutoContrast", "RandomDropFeature",
                                                        "NumpyChromaticNormalize", "RandomJitter", "ChromaticTranslation",
                                                        "ChromaticJitter", "HueSaturationTranslation", "RandomFlip"]})
    rz, sc, ac, df, nm, jt, ct, cj, hs, fl = c.ops
    assert rz.angle == np.pi and rz.rotate_dim == 2 and rz.random_rotate
    assert sc.scale == (0.8, 1.2) and not sc.anisotropic and not sc.use_mirroring and sc.scale_xyz == [True] * 3
    assert ac.p == 0.2 and ac.blend_factor is None and df.p == 0.2 and df.dim == [0, 3] and nm.has == 0
    assert (jt.sigma, jt.clip) == (0.01, 0.05) and (ct.p, ct.ratio) == (0.95, 0.05) and (cj.p, cj.std) == (0.95, 0.005)
    assert (hs.hue_max, hs.saturation_max) == (0.5, 0.2) and fl.p == 0.5
    t = T.TransformChain(["PointsToTensor", "PointCloudScaling", "PointCloudJitter", "PointCloudRotation", "ChromaticDropGPU",
                          "ChromaticNormalize", "PointCloudCenterAndNormalize", "PointCloudTranslation"])
    _, ps, pj, pr, cd, cn, ce, pt = t.ops
    assert (ps.smin, ps.smax) == (np.float32(2. / 3), np.float32(1.5)) and ps.anisotropic and not ps.use_mirroring
    assert (pj.std, pj.clip) == (0.01, 0.05) and pr.angle == [0.0] * 3 and cd.color_drop == 0.2
    assert cn.f[:3] == tuple(float(np.float32(v)) for v in (0.5136457, 0.49523646, 0.44921124))
    assert ce.centering and ce.normalize and ce.g == 2 and pt.shift == [float(np.float32(0.2))] * 2 + [0.0]


def test_kwargs_reach_every_op():
    kw = {"scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02, "color_drop": 0.3, "gravity_dim": 1, "p": 0.7}
    c = T.build_transforms_from_cfg("train", {"train": S3DIS, "kwargs": kw})
    ac, _, ps, al, pr, pj, cd, _ = c.ops
    assert ac.p == 0.7 and (ps.smin, ps.smax) == (np.float32(0.9), np.float32(1.1)) and al.g == 1 and c.gravity_dim == 1
    assert pr.angle == [0.0, 0.0, np.pi] and (pj.std, pj.clip) == (0.005, 0.02) and cd.color_drop == 0.3


@pytest.mark.parametrize("name", ["RandomDropout", "PointCloudToTensor", "RandomShift", "RandomScaleAndTranslate"])
def test_unsupported_transforms_raise_with_the_reason(name):
    with pytest.raises(ValueError, match=name) as e:
        T.build_transforms_from_cfg("train", {"train": ["PointsToTensor", name]})
    assert T.UNSUPPORTED[name] in str(e.value)


def test_other_raises():
    with pytest.raises(KeyError):
        T.build_transforms_from_cfg("train", {"train": ["NoSuchTransform"]})
    with pytest.raises(ValueError, match="compose_fn"):
        T.build_transforms_from_cfg("train", {"train": ["PointsToTensor"], "compose_fn": "ListCompose"})
    with pytest.raises(ValueError, match="PointsToTensor"):
        T.TransformChain(["PointCloudScaling"])  # a torch class on arrays
    with pytest.raises(ValueError, match="numpy"):
        T.TransformChain(["PointsToTensor", "RandomScale"])
    with pytest.raises(ValueError, match=str(T.MAX_OPS)):
        T.TransformChain(["RandomFlip"] * (T.MAX_OPS + 1))
    with pytest.raises(ValueError, match="phases"):
        T.TransformChain(["PointsToTensor"] + ["PointCloudXYZAlign"] * (T.MAX_PHASES + 1))


def test_plan_of_the_s3dis_default_chain():
    p = T.TransformChain(G["meta"]["cases"]["chain_s3dis"]["names"], G["meta"]["cases"]["chain_s3dis"]["kwargs"]).plan()
    assert p["ops"] == S3DIS
    assert [m[0] for m in p["micro"]] == ["AUTOCONTRAST", "SCALE_T", "CENTER", "SUB_MIN_G", "ROT_T", "JITTER_T", "DROP", "NORMALIZE"]
    assert [m[2] for m in p["micro"]] == [0, -1, 0, 0, -1, -1, -1, 1]  # colour and position statistics share phase 0
    assert p["phase_masks"] == [3, 2] and p["phases"] == 2 and p["launches"] <= 1 + p["phases"]
    assert all(d == ("float32", "float32") for d in p["dtypes"]) and p["out_dtype"] == "float32"


def test_plan_of_the_scannet_chains():
    for case, micro in (("chain_scannet", ["ROT_DOT", "SCALE_NP", "AUTOCONTRAST", "DROP", "NORMALIZE"]),
                        ("chain_upstream", ["ROT_DOT", "SCALE_NP", "FLIP_NP", "JITTER_NP", "AUTOCONTRAST", "TRANSLATE_C", "JITTER_C",
                                            "HUESAT", "DROP", "NORMALIZE"])):
        meta = G["meta"]["cases"][case]
        chain = T.TransformChain(meta["names"], meta["kwargs"])
        p = chain.plan()
        assert p["ops"] == meta["names"] and [m[0] for m in p["micro"]] == micro
        assert all(d == ("float64", "float32") for d in p["dtypes"]) and p["out_dtype"] == "float64"  # np.dot comes first
        assert p["phases"] == 2 and p["phase_masks"] == [2, 2] and p["launches"] <= 1 + p["phases"]
        scale = next(m for m in p["_micro"] if m["code"] == "SCALE_NP")
        assert scale["iarg"] & 1  # `pos *= scale` on the float64 array stays float64
    p = T.TransformChain(["RandomScale", "RandomJitter", "RandomRotateZ", "PointsToTensor"]).plan()
    assert [d[0] for d in p["dtypes"]] == ["float32", "float32", "float64", "float32"] and p["phases"] == 0 and p["launches"] == 1
    assert [m["iarg"] & 1 for m in p["_micro"][:2]] == [0, 0] and p["micro"][-1][0] == "TO_F32"
    assert T.TransformChain(["RandomScale"]).plan("float64")["out_dtype"] == "float64"


def test_plan_of_the_centre_and_flip_chain():
    meta = G["meta"]["cases"]["chain_center_flip"]
    p = T.TransformChain(meta["names"], meta["kwargs"]).plan()
    assert [m[0] for m in p["micro"]] == ["AUTOCONTRAST", "SCALE_T", "HFLIP", "HEIGHTS_MIN", "CENTER", "NORM_DIV", "NORMALIZE"]
    # positions: the flip's extrema (0), the mean and gravity minimum of the flipped cloud (1), the largest norm of the centred
    # cloud (2); colours: min / max (0), the maximum after contrast (1)
    assert [m[2] for m in p["micro"]] == [0, -1, 0, 1, 1, 2, 1]
    assert p["phase_masks"] == [3, 3, 1] and p["phases"] == 3 and p["launches"] <= 1 + p["phases"]


def test_draw_spec_names_every_draw_with_its_position():
    c = T.TransformChain(S3DIS, {"angle": [0, 0, 1]})
    assert set(c.spec()) == {"0.u", "0.blend", "2.scale_u", "4.theta", "4.order", "5.noise", "6.u"}
    assert c.spec()["5.noise"][0] == "point" and c.spec()["2.scale_u"][0] == "cloud"
