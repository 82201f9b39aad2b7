"""Records what the reference's own graph convolutions compute on the CPU (models/layers/graph_conv.py):

    python tools/record_graph_conv_fixtures.py   (a fresh process; needs the reference checkout oracle/refshim.py points at)

  tests/golden/graph_conv.npz              per module -- 'edge' (EdgeConv on the k = 9 graph), 'graph' (GraphConv on the
                                           dilation-2 graph), 'dyn_d1' / 'dyn_d2' (DynConv, dilation 1 and 2), 'res'
                                           (ResDynBlock, dilation 2), 'dense' (DenseDynBlock, dilation 1) -- at 2 x 8 x 256,
                                           8 -> 16 channels, BatchNorm + ReLU: the initial state dict, the input, the
                                           edge_index used, the outputs in eval and train mode, the gradients of the input, the
                                           conv weight and the BatchNorm weight under out.square().mean(), and for the train
                                           output and each gradient the largest deviation from the same module run in fp64
  tests/golden/graph_conv_state_keys.json  state-dict keys and shapes per module, in order

Inputs are randint(-512, 512) / 512: every squared distance is a multiple of 2^-18 below 32, exact in fp32 in any evaluation
order.  The recorder asserts that no point has two equal distances among its first k * dilation + 1, so every correct fp32
search returns the recorded lists.

The reference's DenseDynBlock.forward concatenates its (B,C,N,1) input with the squeezed (B,C',N) output, which torch.cat
refuses; for 'dense' the recorder runs the reference's own body (DynConv) and concatenates the four-dimensional tensors.

Only numbers are written: nothing of the reference's program text.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refshim import load_reference  # noqa: E402

load_reference()
from openpoints.models.layers import graph_conv as GC  # noqa: E402  (the reference's)
from openpoints.models.layers.knn import DilatedKNN  # noqa: E402

B, C, N, COUT, K = 2, 8, 256, 16, 9
BLOCK = dict(norm_args={"norm": "bn"}, act_args={"act": "relu"})

g = torch.Generator().manual_seed(23)
x0 = (torch.randint(-512, 512, (B, C, N, 1), generator=g).float() / 512)

d2 = torch.cdist(x0.squeeze(-1).transpose(1, 2).double(), x0.squeeze(-1).transpose(1, 2).double()) ** 2
first = torch.sort(d2, dim=-1).values[..., :K * 2 + 1]
assert bool((first.diff(dim=-1) > 0).all()), "two equal distances among a point's first k * dilation + 1: take another seed"


def static_graph(dilation):
    return DilatedKNN(K, dilation)(x0.squeeze(-1).transpose(1, 2)).int().contiguous()


def _gather_group(features, idx):
    """grouping_operation in plain torch, for any dtype (the shimmed operator takes fp32 only)"""
    b, c = features.shape[:2]
    return features.gather(2, idx.reshape(b, 1, -1).expand(-1, c, -1).long()).reshape(b, c, *idx.shape[1:])


class fp64_operators:
    def __enter__(self):
        self.keep = GC.grouping_operation
        GC.grouping_operation = _gather_group

    def __exit__(self, *exc):
        GC.grouping_operation = self.keep


def dense_forward(m, x):
    try:
        return m(x)
    except RuntimeError:  # the squeezed concatenation: see the module docstring
        return torch.cat((x, m.body(x)), 1)


MODULES = {
    "edge": (lambda: GC.EdgeConv(C, COUT, **BLOCK), 1, True),
    "graph": (lambda: GC.GraphConv(C, COUT, **BLOCK), 2, True),
    "dyn_d1": (lambda: GC.DynConv(C, COUT, k=K, dilation=1, **BLOCK), 1, False),
    "dyn_d2": (lambda: GC.DynConv(C, COUT, k=K, dilation=2, **BLOCK), 2, False),
    "res": (lambda: GC.ResDynBlock(C, k=K, dilation=2, **BLOCK), 2, False),
    "dense": (lambda: GC.DenseDynBlock(C, C + COUT, k=K, dilation=1, **BLOCK), 1, False),
}


def run(tag, m, x, edge_index):
    if edge_index is not None:
        return m(x, edge_index)
    return dense_forward(m, x) if tag == "dense" else m(x)


def train_step(tag, m, x, edge_index):
    m.train()
    m.zero_grad()
    x = x.clone().requires_grad_(True)
    out = run(tag, m, x, edge_index)
    out.square().mean().backward()
    params = dict(m.named_parameters())
    conv = next(k for k in params if k.endswith("nn.0.weight"))
    bn = next(k for k in params if k.endswith("nn.1.weight"))
    return out.detach(), {"x": x.grad, conv: params[conv].grad, bn: params[bn].grad}


out, keys = {"x": x0.numpy(), "meta": np.array([B, C, N, COUT, K])}, {}
for tag, (make, dilation, static) in MODULES.items():
    torch.manual_seed(7)
    m = make()
    sd = copy.deepcopy(m.state_dict())
    keys[tag] = [[k, list(v.shape)] for k, v in sd.items()]
    for k, v in sd.items():
        out[f"{tag}_sd::{k}"] = v.numpy()
    graph = static_graph(dilation)
    out[f"{tag}_edge_index"] = graph.numpy().astype(np.int16)
    if not static:  # the module's own graph is the recorded one
        seen = {}
        knn = (m if tag.startswith("dyn") else m.body).dilated_knn_graph
        knn.register_forward_hook(lambda mod, a, r: seen.__setitem__("idx", r))
    edge_index = graph if static else None
    m.eval()
    with torch.no_grad():
        out[f"{tag}_out_eval"] = run(tag, m, x0, edge_index).numpy()
    twin = copy.deepcopy(m).double()
    y, grads = train_step(tag, m, x0, edge_index)
    if not static:
        assert torch.equal(seen["idx"].int(), graph)
    out[f"{tag}_out_train"] = y.numpy()
    out[f"{tag}_grad_names"] = np.array(list(grads))
    with fp64_operators():
        y64, grads64 = train_step(tag, twin, x0.double(), edge_index)
    out[f"{tag}_fp64_dev::out"] = np.array(float((y.double() - y64).abs().max()))
    for k, v in grads.items():
        out[f"{tag}_grad::{k}"] = v.numpy()
        out[f"{tag}_fp64_dev::{k}"] = np.array(float((v.double() - grads64[k]).abs().max()))
    print(tag, {k.split("::")[-1]: float(v) for k, v in out.items() if k.startswith(f"{tag}_fp64_dev")})

os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "graph_conv.npz"), **out)
with open(os.path.join(ROOT, "tests", "golden", "graph_conv_state_keys.json"), "w") as fh:
    json.dump(keys, fh, indent=0)
print("wrote", sum(v.nbytes for v in out.values()), "bytes of arrays;",
      os.path.getsize(os.path.join(ROOT, "tests", "golden", "graph_conv.npz")), "bytes compressed")
