"""Records tests/golden/s3dis_sphere.npz by RUNNING THE REFERENCE on the CPU (needs the reference tree and sklearn; not run by
the tests):

    python tools/record_sphere_fixtures.py

The reference's own S3DISSphere (openpoints/dataset/s3dis/s3dis_sphere.py) is given a temporary data_root whose
processed/val_<voxel>_data.pkl holds two small synthetic clouds (raw points, sub-points, colours, labels and sklearn KD-trees,
the tuple its __init__ pickles), so that __init__ loads it and computes the schedule table and the projections itself, with its
own KD-tree queries.  np.random is seeded first: the initial potentials are regenerated from the same seed (rand(n) * 1e-3 per
cloud, in order).  A handful of items follow, with np.random.permutation / choice logged.  Stored: the clouds, the initial
potentials, cloud_inds / point_inds / noise of every step, the projections, and per item the draws and every output.
Inputs and numbers only.  The numpy version is recorded: the Tukey weights are float64 with numpy >= 2 (float32 before)."""
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "s3dis_sphere.npz")

from oracle import refshim  # noqa: E402

refshim.load_reference()

from sklearn.neighbors import KDTree  # noqa: E402

from openpoints.dataset.s3dis.s3dis_sphere import S3DISSphere  # noqa: E402  (reference)

VOXEL, RADIUS, NUM_POINTS, STEPS, ITEMS, SEED = 0.04, 1.0, 1024, 24, 8, 20240
SIZES = ((5200, 9000), (3100, 5000))  # (sub-points, raw points) of the two clouds


def make_cloud(n_sub, n_raw, seed, shift):
    """points on the six faces of a box and on a table top inside it, uniformly random (no two distances equal), away from the
    origin; the raw cloud is other random points of the same surfaces"""
    rng = np.random.default_rng(seed)
    size = np.array([2.2, 1.6, 1.1])

    def surface(n):
        face = rng.integers(0, 7, n)
        p = rng.uniform(0, 1, (n, 3)) * size
        for f in range(6):
            p[face == f, f // 2] = (f % 2) * size[f // 2]
        top = face == 6
        p[top] = p[top] * np.array([0.5, 0.5, 0.0]) + np.array([0.6, 0.4, 0.45])
        return (p + rng.normal(0, 0.004, p.shape) + shift).astype(np.float32), face
    sub, face = surface(n_sub)
    raw, raw_face = surface(n_raw)
    colors = np.clip(np.round(rng.uniform(0, 255, (n_sub, 3)) * 0.5 + face[:, None] * 18.0), 0, 255).astype(np.float32)
    labels = ((face * 2 + rng.integers(0, 2, n_sub)) % 13).astype(np.int64)
    raw_labels = ((raw_face * 2 + rng.integers(0, 2, n_raw)) % 13).astype(np.int32).reshape(-1, 1)
    raw_colors = rng.integers(0, 256, (n_raw, 3)).astype(np.float32)
    return sub, colors, labels, raw, raw_colors, raw_labels


def main():
    clouds = [make_cloud(SIZES[0][0], SIZES[0][1], 11, np.array([12.5, -7.25, 0.3])),
              make_cloud(SIZES[1][0], SIZES[1][1], 12, np.array([-3.0, 20.5, 1.0]))]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "processed"))
        trees = [KDTree(c[0], leaf_size=50) for c in clouds]
        with open(os.path.join(tmp, "processed", f"val_{VOXEL:.3f}_data.pkl"), "wb") as f:
            pickle.dump(([c[3] for c in clouds], [c[4] for c in clouds], [c[5] for c in clouds], [[0, len(c[3])] for c in clouds],
                         [c[0] for c in clouds], [c[1] for c in clouds], [c[2] for c in clouds], trees), f)
        np.random.seed(SEED)
        ds = S3DISSphere(VOXEL, RADIUS, NUM_POINTS, STEPS, 1, data_root=tmp, transform=None, split="val")
        np.random.seed(SEED)
        potentials = [np.random.rand(len(c[0])) * 1e-3 for c in clouds]
        assert len(ds.cloud_inds) == STEPS and len(ds) == STEPS
        out["cloud_inds"] = np.array(ds.cloud_inds, dtype=np.int64)
        out["point_inds"] = np.array(ds.point_inds, dtype=np.int64)
        out["noise"] = np.concatenate(ds.noise, 0).astype(np.float64)
        for c, (cl, pot) in enumerate(zip(clouds, potentials)):
            for k, v in zip(("sub_points", "sub_colors", "sub_labels", "points", "labels"), (cl[0], cl[1], cl[2], cl[3], cl[5])):
                out[f"cloud{c}/{k}"] = v
            out[f"cloud{c}/potentials"] = pot
            out[f"cloud{c}/projections"] = np.asarray(ds.projections[c], dtype=np.int32)
        log = []
        orig = np.random.permutation, np.random.choice

        def permutation(x):
            v = orig[0](x)
            log.append(("perm", np.array(v)))
            return v

        def choice(a, size):
            v = orig[1](a, size)
            log.append(("pad", np.array(v)))
            return v
        np.random.permutation, np.random.choice = permutation, choice
        try:
            np.random.seed(SEED + 1)
            curs = []
            for i in range(ITEMS):
                del log[:]
                it = ds[i]
                kinds = [k for k, _ in log]
                assert kinds in (["perm"], ["perm", "pad"]), kinds
                perm = log[0][1].astype(np.int32)
                pad = log[1][1].astype(np.int32) if len(log) == 2 else np.zeros(0, np.int32)
                cur = NUM_POINTS + 1 if len(log) == 1 else len(perm)  # (above num_points the reference does not keep the number)
                curs.append(cur)
                out[f"item{i}/perm"], out[f"item{i}/pad"] = perm, pad
                out[f"item{i}/pos"] = np.asarray(it["pos"], dtype=np.float32)
                out[f"item{i}/x"] = np.asarray(it["x"], dtype=np.float32)
                out[f"item{i}/y"] = np.asarray(it["y"], dtype=np.int64)
                out[f"item{i}/mask"] = it["mask"].numpy().astype(np.int32)
                out[f"item{i}/cloud_index"] = np.int64(it["cloud_index"])
                out[f"item{i}/input_inds"] = np.asarray(it["input_inds"], dtype=np.int64)
                out[f"item{i}/heights"] = it["heights"].numpy().astype(np.float32)
                assert it["pos"].dtype == np.float32 and it["x"].dtype == np.float32 and it["heights"].dtype == torch.float32
        finally:
            np.random.permutation, np.random.choice = orig
    print("clouds of the steps", out["cloud_inds"].tolist())
    print("items: cur (1025 = above num_points)", curs)
    assert any(c > NUM_POINTS for c in curs) and any(c < NUM_POINTS for c in curs), "the items must take both branches"
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__, "voxel_size": VOXEL, "in_radius": RADIUS,
                                       "num_points": NUM_POINTS, "num_steps": STEPS, "items": ITEMS, "seed": SEED, "gravity_dim": 2}))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
