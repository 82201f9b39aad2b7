"""The graph convolutions (models/layers/graph_conv.py) without a GPU: every class is exported, state-dict keys and shapes
are the reference's (tests/golden/graph_conv_state_keys.json, recorded from its own classes by
tools/record_graph_conv_fixtures.py), a CPU forward is refused, the feature-space search is part of the C ABI, and the fp64
restatement the GPU tests compare against orders ties by index."""
import json
import os

import pytest
import torch

import knn_features_ref as R
from conftest import GOLDEN

BLOCK = dict(norm_args={"norm": "bn"}, act_args={"act": "relu"})
C, COUT, K = 8, 16, 9


def make(tag):
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers import DenseDynBlock, DynConv, EdgeConv, GraphConv, ResDynBlock
    return {"edge": lambda: EdgeConv(C, COUT, **BLOCK),
            "graph": lambda: GraphConv(C, COUT, **BLOCK),
            "dyn_d1": lambda: DynConv(C, COUT, k=K, dilation=1, **BLOCK),
            "dyn_d2": lambda: DynConv(C, COUT, k=K, dilation=2, **BLOCK),
            "res": lambda: ResDynBlock(C, k=K, dilation=2, **BLOCK),
            "dense": lambda: DenseDynBlock(C, C + COUT, k=K, dilation=1, **BLOCK)}[tag]()


TAGS = ["edge", "graph", "dyn_d1", "dyn_d2", "res", "dense"]


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "graph_conv_state_keys.json")) as fh:
        return json.load(fh)


def test_every_class_is_exported():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models import layers
    from openpoints.models.layers import graph_conv
    for name in ("MRConv", "EdgeConv", "GraphConv", "DynConv", "ResDynBlock", "DenseDynBlock"):
        assert getattr(layers, name) is getattr(graph_conv, name)
    assert graph_conv.GraphConv(4, 8, conv="mrconv").gconv.__class__ is graph_conv.MRConv
    assert graph_conv.GraphConv(4, 8, conv="edge").gconv.__class__ is graph_conv.EdgeConv


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_is_the_references(keys, tag):
    got = [[k, list(v.shape)] for k, v in make(tag).state_dict().items()]
    assert got == keys[tag]
    assert got[0][1] == [C if tag == "res" else COUT, 2 * C, 1, 1]


def test_mrconv_has_edgeconvs_parameters():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers import EdgeConv, MRConv
    a, b = MRConv(C, COUT, **BLOCK).state_dict(), EdgeConv(C, COUT, **BLOCK).state_dict()
    assert [(k, v.shape) for k, v in a.items()] == [(k, v.shape) for k, v in b.items()]


@pytest.mark.parametrize("tag", TAGS)
def test_cpu_forward_is_refused(tag):
    m = make(tag)
    x = torch.rand(1, C, 32, 1)
    args = (x, torch.zeros(1, 32, K, dtype=torch.int32)) if tag in ("edge", "graph") else (x,)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(*args)


def test_knn_features_refuses_cpu_tensors():
    from amcontrast3d_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.knn_features(3, torch.rand(1, 16, 4))


def test_split_form_is_chosen_from_the_module():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers.graph_conv import EdgeConv, conv_norm_act
    assert [m is not None for m in conv_norm_act(EdgeConv(C, COUT, **BLOCK).nn)] == [True, True, True]
    assert [m is not None for m in conv_norm_act(EdgeConv(C, COUT).nn)] == [True, False, False]
    assert [m is not None for m in conv_norm_act(EdgeConv(C, COUT, act_args={"act": "relu"}).nn)] == [True, False, True]
    assert [m is not None for m in conv_norm_act(EdgeConv(C, COUT, norm_args={"norm": "bn"}).nn)] == [True, True, False]
    assert conv_norm_act(EdgeConv(C, COUT, norm_args={"norm": "bn"}, act_args={"act": "gelu"}).nn) is None
    assert conv_norm_act(EdgeConv(C, COUT, order="conv-act-norm", **BLOCK).nn) is None
    assert conv_norm_act(EdgeConv(C, COUT, norm_args={"norm": "in"}, act_args={"act": "relu"}).nn) is None
    assert EdgeConv(C, COUT, **BLOCK).split_form(torch.rand(1, C, 8, 1)) is None  # a CPU tensor


def test_abi_has_the_feature_search():
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    assert {"amc3d_knn_features", "amc3d_knn_features_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert lib.amc3d_knn_features_workspace_bytes(2, 300, 77, 16, 9) > 0
    assert lib.amc3d_knn_features_workspace_bytes(2, 300, 77, 16, 101) == 0
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amc3d.h")).read()
    assert "int amc3d_knn_features(" in header and "size_t amc3d_knn_features_workspace_bytes(" in header


def test_restatement_orders_ties_by_index():
    sup = torch.tensor([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [3.0, 0.0]]])
    qry = torch.tensor([[[0.0, 0.0]]])
    idx, d2, _ = R.exact_lists(qry, sup, 4)
    assert idx.tolist() == [[[0, 1, 2, 3]]] and d2.tolist() == [[[0.0, 1.0, 1.0, 1.0]]]
    idx, d2, _ = R.exact_lists(qry, sup, 3, farthest=True)
    assert idx.tolist() == [[[4, 1, 2]]] and d2.tolist() == [[[9.0, 1.0, 1.0]]]
    assert float(R.band(qry, sup)[0, 0, 4]) == 2 * 5 * 2.0 ** -24 * 9.0
