"""Records what the reference's own cpp/pointops/functions/pointops.py computes on the CPU, with the NumPy restatements of
tests/pointops_offset_ref.py attached to the `pointops_cuda` stand-in module at run time (k-NN stays the oracle's):

    python tools/record_pointops_fixtures.py        (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/pointops_offset.npz               inputs, outputs and gradients of every public function on one ragged batch
                                                 (support segments 1, 2, 65, 300, 7; query segments 1, 1, 20, 75, 3)
  tests/golden/pointops_offset_signatures.json   parameter names and defaults of every public callable of the module

Only numbers and names are written: nothing of the reference's program text.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refshim import load_reference  # noqa: E402

load_reference()
import pointops_cuda  # noqa: E402  (the oracle's stand-in: knnquery_cuda)
import pointops_offset_ref as R  # noqa: E402

stand_in = R.as_pointops_cuda()
for name in R.ENTRY_POINTS:
    if name != "knnquery_cuda":
        setattr(pointops_cuda, name, getattr(stand_in, name))
from openpoints.cpp.pointops.functions import pointops as P  # noqa: E402  (the reference's)

SEG, QSEG = [1, 2, 65, 300, 7], [1, 1, 20, 75, 3]
C, NS, WC, K = 6, 5, 3, 3
RADIUS = 0.3

g = torch.Generator().manual_seed(7)
xyz = torch.from_numpy(np.concatenate([R.cloud(21 + i, c, "uniform") for i, c in enumerate(SEG)]))
offset, new_offset = torch.from_numpy(R.ends(SEG)), torch.from_numpy(R.ends(QSEG))
n, m = xyz.shape[0], int(new_offset[-1])
feat = torch.randn(n, C, generator=g)
out = {"xyz": xyz.numpy(), "offset": offset.numpy(), "new_offset": new_offset.numpy(), "feat": feat.numpy(),
       "meta": json.dumps({"c": C, "nsample": NS, "w_c": WC, "k": K, "radius": RADIUS})}


def rand(*shape):
    return torch.randn(*shape, generator=g)


def leaf(t):
    return t.clone().requires_grad_(True)


def run(key, fn, leaves, seed_grads=True):
    """fn(*leaves) -> tensor or tuple of tensors; records outputs, the upstream gradients drawn for them and the leaves' grads"""
    leaves = [leaf(t) for t in leaves]
    res = fn(*leaves)
    res = res if isinstance(res, tuple) else (res,)
    ups = [rand(*r.shape) for r in res]
    pairs = [(r, u) for r, u in zip(res, ups) if r.requires_grad]
    torch.autograd.backward([r for r, _ in pairs], [u for _, u in pairs])
    for i, (r, u) in enumerate(zip(res, ups)):
        out[f"{key}/out{i}"], out[f"{key}/up{i}"] = r.detach().numpy(), u.numpy()
    for i, t in enumerate(leaves):
        out[f"{key}/grad{i}"] = t.grad.numpy()


fps = P.furthestsampling(xyz, offset, new_offset)
out["furthestsampling/idx"] = fps.numpy()
new_xyz = xyz[fps.long()].contiguous()
out["new_xyz"] = new_xyz.numpy()
knn_idx, knn_dist = P.knnquery(NS, xyz, new_xyz, offset, new_offset)
out["knnquery/idx"], out["knnquery/dist"] = knn_idx.numpy(), knn_dist.numpy()
ball_idx = P.ballquery(RADIUS, NS, xyz, new_xyz, offset, new_offset)
out["ballquery/idx"] = ball_idx.numpy()
self_idx, _ = P.knnquery(NS, xyz, xyz, offset, offset)  # (n, NS): the neighbourhoods of subtraction / aggregation
out["self_idx"] = self_idx.numpy()

run("grouping", lambda f: P.grouping(f, ball_idx), [feat])
for method, radius in (("knn", None), ("knnquery", RADIUS), ("ballquery", RADIUS)):  # 'knnquery' normalises by the radius
    for norm in (False, True):
        run(f"querygroup/{method}/{int(norm)}",
            lambda f: P.querygroup(NS, xyz, new_xyz, f, offset, new_offset, radius=radius, query_method=method, normalize_dp=norm),
            [feat])
run("querygroup_xyz", lambda x, f: P.querygroup(NS, x, new_xyz, f, offset, new_offset), [xyz, feat])
for use_xyz in (True, False):
    run(f"queryandgroup/{int(use_xyz)}", lambda f: P.queryandgroup(NS, xyz, new_xyz, f, None, offset, new_offset, use_xyz=use_xyz),
        [feat])
run("queryandgroup_idx", lambda f: P.queryandgroup(NS, xyz, new_xyz, f, ball_idx, offset, new_offset), [feat])

feat2 = rand(n, C)
position, weight = rand(n, NS, C), rand(n, NS, WC)
out["feat2"], out["position"], out["weight"] = feat2.numpy(), position.numpy(), weight.numpy()
run("subtraction", lambda a, b: P.subtraction(a, b, self_idx), [feat, feat2])
run("aggregation", lambda f, p, w: P.aggregation(f, p, w, self_idx), [feat, position, weight])

# interpolation: from the m sampled rows (support) up to all n rows
feat_m = rand(m, C)
out["feat_m"] = feat_m.numpy()
run("interpolation", lambda f: P.interpolation(new_xyz, xyz, f, new_offset, offset, k=K), [feat_m])
run("interpolation2", lambda f: P.interpolation2(new_xyz, xyz, f, new_offset, offset, K), [feat_m])
up_idx, up_dist = P.knnquery(K, new_xyz, xyz, new_offset, offset)
out["interpolation/idx"], out["interpolation/dist"] = up_idx.numpy(), up_dist.numpy()

golden = os.path.join(ROOT, "tests", "golden")
np.savez_compressed(os.path.join(golden, "pointops_offset.npz"), **out)


def params(fn, drop_first=False):
    ps = list(inspect.signature(fn).parameters.values())[1 if drop_first else 0:]
    return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in ps]


sig = {}
for name, obj in sorted(vars(P).items()):
    owner = getattr(obj, "__self__", obj)  # X.apply is a bound method of X
    if name.startswith("_") or inspect.ismodule(obj) or getattr(owner, "__module__", None) != P.__name__:
        continue  # what the module imports (torch, Function, Tuple, nn) is not its surface
    if inspect.isclass(obj):
        sig[name] = {"kind": "Function", "forward": params(obj.forward, drop_first=True)}
    elif inspect.isfunction(obj):
        sig[name] = {"kind": "function", "params": params(obj)}
    elif callable(obj):  # X.apply
        sig[name] = {"kind": "apply", "of": obj.__self__.__name__}
with open(os.path.join(golden, "pointops_offset_signatures.json"), "w") as f:
    json.dump(sig, f, indent=1, sort_keys=True)
print(len(out), "arrays;", sorted(sig))
