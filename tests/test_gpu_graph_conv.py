"""models/layers/graph_conv.py on the GPU against what the reference's own classes computed on the CPU
(tests/golden/graph_conv.npz, tools/record_graph_conv_fixtures.py: 2 x 8 x 256, 8 -> 16 channels, k = 9, dilation 1 and 2).

Margins.  Outputs: 1e-4 absolute on the BatchNorm-scaled values (the project's margin for logits).  Gradients: 4 x the
deviation of the reference's own fp32 run from its fp64 twin, recorded per tensor in the fixture, plus 1e-6 of the tensor's
largest entry: the reference's rounding is the yardstick, and the split form of EdgeConv adds its sums in another order.
The fixture's inputs are multiples of 1/512, so all squared distances are exact in fp32 and no point has two equal ones
among its first k * dilation + 1: DynConv's own graph must equal the recorded one at every point."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_graph_conv_host import BLOCK, C, COUT, K, make

pytestmark = pytest.mark.gpu

STATIC, DYNAMIC = ["edge", "graph"], ["dyn_d1", "dyn_d2", "res", "dense"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(GOLDEN, "graph_conv.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def loaded(fix, tag, dev):
    m = make(tag)
    sd = {k.split("::", 1)[1]: torch.from_numpy(v) for k, v in fix.items() if k.startswith(f"{tag}_sd::")}
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def dyn_of(m):
    return m if hasattr(m, "dilated_knn_graph") else m.body


def call(m, tag, x, fix, dev):
    if tag in STATIC:
        return m(x, torch.from_numpy(fix[f"{tag}_edge_index"].astype(np.int32)).to(dev))
    return m(x)


@pytest.mark.parametrize("tag", STATIC + DYNAMIC)
def test_outputs_and_gradients_match_the_reference(fix, dev, tag):
    m = loaded(fix, tag, dev)
    x = torch.from_numpy(fix["x"]).to(dev)
    m.eval()
    with torch.no_grad():
        got = call(m, tag, x, fix, dev)
    err = float((got.cpu() - torch.from_numpy(fix[f"{tag}_out_eval"])).abs().max())
    print(f"{tag}: eval output off by {err:.2e}")
    assert got.shape == fix[f"{tag}_out_eval"].shape and err <= 1e-4

    m.train()
    xg = x.clone().requires_grad_(True)
    out = call(m, tag, xg, fix, dev)
    out.square().mean().backward()
    err = float((out.detach().cpu() - torch.from_numpy(fix[f"{tag}_out_train"])).abs().max())
    print(f"{tag}: train output off by {err:.2e}")
    assert err <= 1e-4
    grads = {"x": xg.grad, **{k: p.grad for k, p in m.named_parameters()}}
    for name in fix[f"{tag}_grad_names"].tolist():
        want = torch.from_numpy(fix[f"{tag}_grad::{name}"])
        margin = 4 * float(fix[f"{tag}_fp64_dev::{name}"]) + 1e-6 * float(want.abs().max())
        err = float((grads[name].cpu() - want).abs().max())
        print(f"{tag}: gradient of {name} off by {err:.3e}, margin {margin:.3e}")
        assert err <= margin, name


@pytest.mark.parametrize("tag", DYNAMIC)
def test_dynconv_builds_the_recorded_graph(fix, dev, tag):
    m = dyn_of(loaded(fix, tag, dev))
    got = m.graph(torch.from_numpy(fix["x"]).to(dev))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(fix[f"{tag}_edge_index"].astype(np.int32)))


@pytest.mark.parametrize("training", [False, True])
def test_dynconv_is_graphconv_on_its_own_graph(fix, dev, training):
    from openpoints.models.layers import GraphConv
    x = torch.from_numpy(fix["x"]).to(dev)
    a, b = loaded(fix, "dyn_d2", dev).train(training), loaded(fix, "dyn_d2", dev).train(training)
    with torch.no_grad():
        assert torch.equal(a(x), GraphConv.forward(b, x, b.graph(x)))


def test_stochastic_pick_draws_as_densedilated_does(fix, dev):
    from amcontrast3d_amd import ops
    from openpoints.models.layers import DenseDilated, DynConv
    x = torch.from_numpy(fix["x"]).to(dev)
    feats = x.squeeze(-1).contiguous()
    full = ops.knn_features(2 * K, feats, channel_major=True)[1]
    for eps, training in ((1.0, True), (0.0, True), (1.0, False)):
        m = DynConv(C, COUT, k=K, dilation=2, stochastic=True, epsilon=eps, **BLOCK).to(dev).train(training)
        torch.manual_seed(3)
        got = m.graph(x)
        after = torch.get_rng_state()
        torch.manual_seed(3)
        randnum = DenseDilated(K, 2, True, eps).train(training).draw()
        assert torch.equal(after, torch.get_rng_state())
        assert (randnum is not None) == (eps == 1.0 and training)
        want = full[:, :, randnum.to(dev)] if randnum is not None else full[:, :, ::2]
        assert torch.equal(got, want)


def edge_statement(m, x, idx):
    """max_k nn([x_i ; x_j - x_i]) in fp64 on the CPU, the module's own block"""
    nn64 = copy.deepcopy(m.nn).double().cpu()
    x, idx = x.double().cpu(), idx.cpu().long()
    b, c, n, _ = x.shape
    xj = x.squeeze(-1).gather(2, idx.reshape(b, 1, -1).expand(-1, c, -1)).reshape(b, c, n, -1)
    return nn64(torch.cat([x.expand(-1, -1, -1, idx.shape[-1]), xj - x], 1)).max(-1, keepdim=True)[0]


@pytest.mark.parametrize("kwargs,split", [(BLOCK, True), (dict(act_args={"act": "relu"}), True), (dict(), True),
                                          (dict(norm_args={"norm": "bn"}), True),
                                          (dict(norm_args={"norm": "bn"}, act_args={"act": "gelu"}), False),
                                          (dict(order="conv-act-norm", **BLOCK), False)])
def test_split_form_follows_the_block(fix, dev, kwargs, split):
    from amcontrast3d_amd import timing
    from openpoints.models.layers import EdgeConv
    torch.manual_seed(5)
    m = EdgeConv(C, COUT, **kwargs).to(dev).train()
    x = torch.from_numpy(fix["x"]).to(dev)
    idx = torch.from_numpy(fix["edge_edge_index"].astype(np.int32)).to(dev)
    want = edge_statement(m, x, idx)
    with timing.count_calls() as calls:
        got = m(x, idx)
    assert calls["pointwise_conv_forward"] == (1 if split else 0)
    assert calls["group_points"] == 1
    err = float((got.detach().cpu().double() - want).abs().max())
    print(f"{kwargs}: off by {err:.2e}")
    assert got.shape == (2, COUT, 256, 1) and err <= 1e-4


def test_mrconv_is_the_max_relative_convolution(fix, dev):
    from openpoints.models.layers import MRConv
    torch.manual_seed(5)
    m = MRConv(C, COUT, **BLOCK).to(dev).train()
    x = torch.from_numpy(fix["x"]).to(dev)
    idx = torch.from_numpy(fix["edge_edge_index"].astype(np.int32)).to(dev)
    nn64 = copy.deepcopy(m.nn).double().cpu()
    got = m(x, idx)
    x64, i64 = x.double().cpu(), idx.cpu().long()
    xj = x64.squeeze(-1).gather(2, i64.reshape(2, 1, -1).expand(-1, C, -1)).reshape(2, C, 256, K)
    want = nn64(torch.cat([x64, xj.max(-1, keepdim=True)[0] - x64], 1))
    assert got.shape == (2, COUT, 256, 1) and float((got.detach().cpu().double() - want).abs().max()) <= 1e-4


def test_dynconv_forward_has_one_search_and_no_distance_matrix(dev):
    from amcontrast3d_amd import timing
    from openpoints.models.layers import DynConv
    N = 4096
    torch.manual_seed(1)
    m = DynConv(C, COUT, k=K, dilation=1, **BLOCK).to(dev).train()
    x = torch.randn(1, C, N, 1, device=dev)
    with torch.no_grad():
        m(x)  # workspaces of the first call
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with timing.count_calls() as calls:
            y = m(x)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
    print(f"peak memory grew by {grown} bytes; N * N = {N * N}")
    assert calls["knn_features"] == 1 and calls["knn_batch"] == 0
    assert y.shape == (1, COUT, N, 1) and grown < N * N
