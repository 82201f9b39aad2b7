"""Records what the reference's own k-NN modules compute on the CPU (models/layers/knn.py and group.py):

    python tools/record_knn_group_fixtures.py       (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/knn_group.npz   B = 2, support 300, queries 77, k = 9 and 9 x 2, C = 5: knn_point, both KNN modules
                               (farthest=True once), DilatedKNN plain and stochastic (training, epsilon = 1, seeded),
                               KNNGroup over relative_xyz x normalize_dp, with and without features, return_only_idx;
                               and a self-search of 2 x 2048 points at k = 16

Only numbers are written: nothing of the reference's program text.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refshim import load_reference  # noqa: E402

load_reference()
from openpoints.models.layers import group as G  # noqa: E402  (the reference's)
from openpoints.models.layers import knn as Kn  # noqa: E402

B, N, M, K, D, C, NSELF, KSELF, SEED = 2, 300, 77, 9, 2, 5, 2048, 16, 5
rng = np.random.default_rng(3)
sup = torch.from_numpy(rng.uniform(0, 2, size=(B, N, 3)).astype(np.float32))
qry = torch.from_numpy(rng.uniform(0, 2, size=(B, M, 3)).astype(np.float32))
feat = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32))
big = torch.from_numpy(rng.uniform(0, 2, size=(B, NSELF, 3)).astype(np.float32))
out = {"sup": sup.numpy(), "qry": qry.numpy(), "feat": feat.numpy(), "big": big.numpy(),
       "meta": np.array([B, N, M, K, D, C, NSELF, KSELF, SEED])}


def put(name, t, small=False):
    a = t.detach().numpy()
    out[name] = a.astype(np.int16) if small else a
    out[name + "_dtype"] = np.array(str(t.dtype))


v, i = Kn.knn_point(K, qry, sup)
put("point_val", v); put("point_idx", i)
v, i = Kn.KNN(K)(qry, sup)
put("knn_val", v); put("knn_idx", i)
v, i = Kn.KNN(K, farthest=True)(qry, sup)
put("far_val", v); put("far_idx", i)
v, i = G.KNN(K)(sup, qry)
put("gknn_val", v); put("gknn_idx", i)
for tag, mod in (("knn", Kn), ("group", G)):
    put(f"dil_{tag}", mod.DilatedKNN(K, D)(sup))
    sto = mod.DilatedKNN(K, D, stochastic=True, epsilon=1.0).train()
    torch.manual_seed(SEED)
    put(f"sto_{tag}", sto(sup))
put("only_idx", G.KNNGroup(K, return_only_idx=True)(qry, sup, feat))
for rel in (0, 1):
    for norm in (0, 1):
        dp, fj = G.KNNGroup(K, relative_xyz=bool(rel), normalize_dp=bool(norm))(qry, sup, feat)
        put(f"dp_r{rel}_n{norm}", dp)
        dp0, none = G.KNNGroup(K, relative_xyz=bool(rel), normalize_dp=bool(norm))(qry, sup)
        assert none is None and torch.equal(dp0, dp)
put("fj", fj)
_, i = G.KNN(KSELF)(big, big)
put("big_idx", i, small=True)

path = os.path.join(ROOT, "tests", "golden", "knn_group.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
