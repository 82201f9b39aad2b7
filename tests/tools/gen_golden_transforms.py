"""Records tests/golden/transforms.npz by RUNNING THE REFERENCE's transform classes on the CPU (needs the reference tree; not run
by the tests):

    python tests/tools/gen_golden_transforms.py

Every class amcontrast3d_amd.transforms supports runs alone (a torch class behind PointsToTensor, which it needs), and four
chains run whole: the S3DIS default, the ScanNet default, an upstream-style ScanNet chain and one with
PointCloudCenterAndNormalize and RandomHorizontalFlip.  Each case runs on five small clouds (1, 63, 64, 65 and 777 points in a
6 m box, colours 0..255; the 63-point cloud has a constant blue channel, so the reference's own 255 / 0 comes through).  Every
random number is logged by wrapping random.random, the np.random functions and torch.rand / randn_like, the rotation matrices by
wrapping np.dot and torch.tensor.  Seeds are searched per cloud until the probability-gated branches of the case are recorded
all taken (cloud 0), all not taken (clouds 1 and 2; on the constant-colour cloud 1 ChromaticAutoContrast is taken instead,
unless a HueSaturationTranslation follows, whose uint8 casts of NaN are not defined) and as they fall (clouds 3, 4).

Stored: the inputs once, and per case and cloud the draws under the keys of TransformChain.draw and the outputs (pos / x only
where the case changes them, heights only where a class sets it).  Data only."""
import collections
import collections.abc
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "transforms.npz")

from oracle import refshim  # noqa: E402

refshim.load_reference()
if not hasattr(collections, "Iterable"):
    collections.Iterable = collections.abc.Iterable  # removed from `collections` in Python 3.10; PointCloudRotation reads it

from openpoints.transforms import build_transforms_from_cfg  # noqa: E402  (reference)
from openpoints.utils import EasyConfig  # noqa: E402

SIZES = [1, 63, 64, 65, 777]
S3DIS_KW = {"color_drop": 0.2, "gravity_dim": 2, "scale": [0.9, 1.1], "angle": [0, 0, 1], "jitter_sigma": 0.005, "jitter_clip": 0.02}
SCANNET_KW = {"color_drop": 0.2, "gravity_dim": 2, "rotate_dim": 2, "scale": [0.8, 1.2], "mirror": [0.2, -1, -1], "angle": 1,
              "color_mean": [0.46259782, 0.46253258, 0.46253258], "color_std": [0.693565, 0.6852543, 0.68061745]}  # cfgs/scannet/default.yaml
T = "PointsToTensor"
CASES = {
    # the numpy classes alone
    "PointsToTensor": ([T], {}),
    "RandomRotate": (["RandomRotate"], {"angle": [0.1, 0.2, 1]}),
    "RandomRotateZ": (["RandomRotateZ"], {"angle": 1.0, "rotate_dim": 2}),
    "RandomScale": (["RandomScale"], {"scale": [0.8, 1.2], "scale_anisotropic": True, "mirror": [0.5, 0.5, -1], "scale_xyz": [True, True, False]}),
    "RandomScaleAndJitter": (["RandomScaleAndJitter"], {"scale": [0.8, 1.2], "jitter_sigma": 0.01, "jitter_clip": 0.02}),
    "RandomFlip": (["RandomFlip"], {"p": 0.5}),
    "RandomJitter": (["RandomJitter"], {"jitter_sigma": 0.01, "jitter_clip": 0.02}),
    "ChromaticAutoContrast": (["ChromaticAutoContrast"], {"p": 0.2}),
    "ChromaticTranslation": (["ChromaticTranslation"], {"p": 0.95, "ratio": 0.05}),
    "ChromaticJitter": (["ChromaticJitter"], {"p": 0.95, "std": 0.005}),
    "HueSaturationTranslation": (["HueSaturationTranslation"], {"hue_max": 0.5, "saturation_max": 0.2}),
    "RandomDropFeature": (["RandomDropFeature"], {"feature_drop": 0.2}),
    "NumpyChromaticNormalize": (["NumpyChromaticNormalize"], {"color_mean": [0.46, 0.45, 0.4], "color_std": [0.27, 0.26, 0.28]}),
    # the torch classes behind PointsToTensor
    "PointCloudCenterAndNormalize": ([T, "PointCloudCenterAndNormalize"], {"gravity_dim": 2}),
    "PointCloudXYZAlign": ([T, "PointCloudXYZAlign"], {"gravity_dim": 2}),
    "RandomHorizontalFlip": ([T, "RandomHorizontalFlip"], {"upright_axis": "z", "aug_prob": 0.95}),
    "PointCloudScaling": ([T, "PointCloudScaling"], {"scale": [0.9, 1.1], "mirror": [0.5, 0, 0]}),
    "PointCloudTranslation": ([T, "PointCloudTranslation"], {"shift": [0.2, 0.2, 0.]}),
    "PointCloudScaleAndTranslate": ([T, "PointCloudScaleAndTranslate"], {"scale": [0.9, 1.1], "shift": [0.2, 0.2, 0.2]}),
    "PointCloudJitter": ([T, "PointCloudJitter"], {"jitter_sigma": 0.005, "jitter_clip": 0.02}),
    "PointCloudScaleAndJitter": ([T, "PointCloudScaleAndJitter"], {"scale": [0.9, 1.1], "mirror": [1, 0, 0], "jitter_sigma": 0.005, "jitter_clip": 0.02}),
    "PointCloudRotation": ([T, "PointCloudRotation"], {"angle": [0.05, 0.1, 1]}),
    "ChromaticDropGPU": ([T, "ChromaticDropGPU"], {"color_drop": 0.2}),
    "ChromaticPerDropGPU": ([T, "ChromaticPerDropGPU"], {"color_drop": 0.2}),
    "ChromaticNormalize": ([T, "ChromaticNormalize"], {}),
    # whole chains
    "chain_s3dis": (["ChromaticAutoContrast", T, "PointCloudScaling", "PointCloudXYZAlign", "PointCloudRotation", "PointCloudJitter",
                     "ChromaticDropGPU", "ChromaticNormalize"], S3DIS_KW),  # cfgs/s3dis/default.yaml
    "chain_scannet": (["RandomRotateZ", "RandomScale", "ChromaticAutoContrast", "RandomDropFeature", "NumpyChromaticNormalize"],
                      SCANNET_KW),  # cfgs/scannet/default.yaml
    "chain_upstream": (["RandomRotateZ", "RandomScale", "RandomFlip", "RandomJitter", "ChromaticAutoContrast", "ChromaticTranslation",
                        "ChromaticJitter", "HueSaturationTranslation", "RandomDropFeature", "NumpyChromaticNormalize"], SCANNET_KW),
    "chain_center_flip": (["ChromaticAutoContrast", T, "PointCloudScaling", "RandomHorizontalFlip", "PointCloudCenterAndNormalize",
                           "ChromaticNormalize"], dict(S3DIS_KW, upright_axis="z")),
}
NP_NAMES = ("rand", "uniform", "randn", "shuffle")
CUR = {"n": 0}


def make_cloud(n, seed, constant_blue):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 6.0, (n, 3)).astype(np.float32)
    x = np.round(rng.uniform(0.0, 255.0, (n, 3))).astype(np.float32)
    if constant_blue:
        x[:, 2] = 117.0
    return pos, x


def run_logged(tf, pos, x, seed):
    """the transform on one cloud from one seed, every draw logged in order -> (data, log)"""
    log = []
    orig_np = {n: getattr(np.random, n) for n in NP_NAMES}
    orig = (random.random, torch.rand, torch.randn_like, np.dot, torch.tensor)

    def np_wrap(n):
        def f(*a, **k):
            if n == "shuffle":
                before = list(a[0])
                orig_np[n](*a, **k)
                log.append(("np.shuffle", np.array([next(j for j, m in enumerate(before) if m is e) for e in a[0]], np.int64)))
                return None
            v = orig_np[n](*a, **k)
            log.append(("np." + n, np.array(v)))
            return v
        return f

    def t_wrap(name, fn):
        def f(*a, **k):
            v = fn(*a, **k)
            log.append((name, v.clone().numpy()))
            return v
        return f

    def py_random():
        v = orig[0]()
        log.append(("random.random", np.float64(v)))
        return v

    def dot(a, b, *r, **k):
        if np.shape(a) == (CUR["n"], 3) and np.shape(b) == (3, 3):
            log.append(("np.dot", np.array(b, np.float64)))
        return orig[3](a, b, *r, **k)

    def tensor(a, *r, **k):
        if isinstance(a, np.ndarray) and a.shape == (3, 3):
            log.append(("torch.tensor", np.array(a, np.float64)))
        return orig[4](a, *r, **k)

    for n in NP_NAMES:
        setattr(np.random, n, np_wrap(n))
    random.random, torch.rand, torch.randn_like = py_random, t_wrap("torch.rand", orig[1]), t_wrap("torch.randn_like", orig[2])
    np.dot, torch.tensor = dot, tensor
    try:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        CUR["n"] = len(pos)
        with np.errstate(all="ignore"):
            data = tf({"pos": pos.copy(), "x": x.copy()})
    finally:
        for n in NP_NAMES:
            setattr(np.random, n, orig_np[n])
        random.random, torch.rand, torch.randn_like, np.dot, torch.tensor = orig
    return data, log


def parse(names, kw, log, n):
    """the draws under TransformChain.draw's keys, and the gates (op index, taken) in chain order"""
    it = iter(log)

    def take(kind):
        k, v = next(it)
        assert k == kind, (k, kind)
        return v
    d, gates = {}, []
    g = lambda name, default: kw.get(name, default)  # noqa: E731
    for i, name in enumerate(names):
        p = f"{i}."
        if name == "RandomRotate":
            d[p + "angle"] = np.array([take("np.uniform") for _ in range(3)], np.float64)
            d[p + "R"] = np.ascontiguousarray(take("np.dot").T)
        elif name == "RandomRotateZ":
            d[p + "angle"] = np.float64(take("np.uniform"))
            d[p + "R"] = take("np.dot")
        elif name in ("RandomScale", "RandomScaleAndJitter"):
            d[p + "scale"] = take("np.uniform").astype(np.float64).reshape(-1)
            if (np.array(g("mirror", [-1, -1, -1])) > 0).any():
                d[p + "mirror_u"] = take("np.rand")
            if name == "RandomScaleAndJitter":
                d[p + "noise"] = take("np.randn")
        elif name == "RandomFlip":
            d[p + "u"] = np.array([take("np.rand"), take("np.rand")], np.float64)
            gates += [(i, bool(v < g("p", 0.5))) for v in d[p + "u"]]
        elif name == "RandomJitter":
            d[p + "noise"] = take("np.randn")
        elif name == "ChromaticAutoContrast":
            d[p + "u"] = np.float64(take("np.rand"))
            taken = bool(d[p + "u"] < g("p", 0.2))
            d[p + "blend"] = np.float64(take("np.rand")) if taken and g("blend_factor", None) is None else np.float64(0.0)
            gates.append((i, taken))
        elif name == "ChromaticTranslation":
            d[p + "u"] = np.float64(take("np.rand"))
            taken = bool(d[p + "u"] < g("p", 0.95))
            d[p + "tr_u"] = take("np.rand").reshape(3) if taken else np.zeros(3)
            gates.append((i, taken))
        elif name == "ChromaticJitter":
            d[p + "u"] = np.float64(take("np.rand"))
            taken = bool(d[p + "u"] < g("p", 0.95))
            d[p + "noise"] = take("np.randn") if taken else np.zeros((n, 3))
            gates.append((i, taken))
        elif name == "HueSaturationTranslation":
            d[p + "hue_u"], d[p + "sat_u"] = np.float64(take("np.rand")), np.float64(take("np.rand"))
        elif name == "RandomDropFeature":
            d[p + "u"] = np.float64(take("np.rand"))
            gates.append((i, bool(d[p + "u"] < g("feature_drop", 0.2))))
        elif name == "RandomHorizontalFlip":
            u = [take("random.random")]
            taken = bool(u[0] < g("aug_prob", 0.95))
            u += [take("random.random"), take("random.random")] if taken else [1.0, 1.0]
            d[p + "u"] = np.array(u, np.float64)
            gates += [(i, taken), (i, bool(u[1] < 0.5)), (i, bool(u[2] < 0.5))]
        elif name in ("PointCloudScaling", "PointCloudScaleAndTranslate", "PointCloudScaleAndJitter"):
            d[p + "scale_u"] = take("torch.rand")
            if name == "PointCloudScaleAndJitter" or (np.array(g("mirror", [0, 0, 0])) > 0).any():
                d[p + "mirror_u"] = take("torch.rand")
            if name == "PointCloudScaleAndTranslate":
                d[p + "shift_u"] = take("torch.rand")
            if name == "PointCloudScaleAndJitter":
                d[p + "noise"] = take("torch.randn_like")
        elif name == "PointCloudTranslation":
            d[p + "u"] = take("torch.rand")
        elif name == "PointCloudJitter":
            d[p + "noise"] = take("torch.randn_like")
        elif name == "PointCloudRotation":
            d[p + "theta"] = np.array([take("np.uniform") for _ in range(3)], np.float64)
            d[p + "order"] = take("np.shuffle")
            d[p + "R"] = take("torch.tensor")
        elif name == "ChromaticDropGPU":
            d[p + "u"] = np.float32(take("torch.rand")[0])
            gates.append((i, bool(d[p + "u"] < np.float32(g("color_drop", 0.2)))))
        elif name == "ChromaticPerDropGPU":
            d[p + "noise"] = take("torch.rand").reshape(-1)
    assert next(it, None) is None, [k for k, _ in log]
    return d, gates


def wanted(names, cloud, gates):
    """does this seed give the branches the cloud is to record?"""
    if cloud >= 3 or not gates:
        return True
    if cloud == 0:
        return all(t for _, t in gates)
    contrast_on = cloud == 1 and "HueSaturationTranslation" not in names
    return all(t == (contrast_on and names[i] == "ChromaticAutoContrast") for i, t in gates)


def to_np(v):
    return v.numpy() if torch.is_tensor(v) else np.asarray(v)


def main():
    out, meta = {}, {"numpy": np.__version__, "torch": torch.__version__, "sizes": SIZES, "cases": {}}
    clouds = [make_cloud(n, 100 + c, c == 1) for c, n in enumerate(SIZES)]
    for c, (pos, x) in enumerate(clouds):
        out[f"in/{c}/pos"], out[f"in/{c}/x"] = pos, x
    for case, (names, kw) in CASES.items():
        cfg = EasyConfig()
        cfg.update({"train": names, "kwargs": kw})
        tf = build_transforms_from_cfg("train", cfg)
        seen = {}
        for c, (pos, x) in enumerate(clouds):
            for seed in range(200000):
                data, log = run_logged(tf, pos, x, seed)
                d, gates = parse(names, kw, log, len(pos))
                if wanted(names, c, gates):
                    break
            else:
                raise RuntimeError(f"{case}: no seed gives cloud {c} its branches")
            for j, (_, t) in enumerate(gates):
                seen.setdefault(j, set()).add(t)
            po, xo = to_np(data["pos"]), to_np(data["x"])
            assert xo.dtype == np.float32 and po.dtype in (np.float32, np.float64)
            out[f"{case}/{c}/pos_dtype"] = np.array(str(po.dtype))
            if not (po.dtype == pos.dtype and np.array_equal(po, pos)):
                out[f"{case}/{c}/pos"] = po
            if not np.array_equal(xo, x, equal_nan=True):
                out[f"{case}/{c}/x"] = xo
            if "heights" in data:
                out[f"{case}/{c}/heights"] = to_np(data["heights"]).astype(np.float32)
            for key, v in d.items():
                out[f"{case}/{c}/d/{key}"] = np.asarray(v)
        assert all(s == {True, False} for s in seen.values()), (case, seen)
        meta["cases"][case] = {"names": names, "kwargs": kw}
        print(case, "gates", len(seen))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
