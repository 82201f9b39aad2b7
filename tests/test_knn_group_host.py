"""The k-NN grouper without a GPU: the registry and the exported names, the torch route of every module against what the
reference's own classes computed (tests/golden/knn_group.npz, tools/record_knn_group_fixtures.py), and the yardstick
the GPU tests use -- the oracle's pointops k-NN -- against the exact fp64 neighbour lists.

Index lists are compared with the reference's only for queries whose FIXTURE list is the exact fp64 list: cdist + topk
rounds (its lists are not the nearest points for 0.15-0.25 % of the queries of the 2 x 2048 self-search at k = 16, none
of the 300 / 77 case, measured when the fixture was recorded), and a query it got wrong says nothing about the code under
test.  The share left out may be at most 1 %."""
import os

import numpy as np
import pytest
import torch

import knn_group_ref as R
from conftest import GOLDEN
from test_gpu_ops import clouds


@pytest.fixture(scope="module")
def fix():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    z = np.load(os.path.join(GOLDEN, "knn_group.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    for k in ("sup", "qry", "feat", "big"):
        d[k] = torch.from_numpy(d[k])
    d["exact"], d["untied"] = R.exact_knn(18, d["qry"], d["sup"])
    return d


def _agree(fixture_idx, exact_idx):
    """(B,M) bool: the fixture's list is the exact one; at most 1 % of the queries may be left out"""
    ok = (torch.as_tensor(fixture_idx).long() == exact_idx).all(dim=-1)
    share = 1.0 - float(ok.float().mean())
    print(f"share of queries whose reference list is not the exact list: {share:.4%}")
    assert share <= 0.01, share
    return ok


def test_create_grouper_knn():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models.layers import create_grouper
    from openpoints.models.layers.group import KNNGroup, QueryAndGroup
    g = create_grouper({'NAME': 'knn', 'nsample': 16})
    assert isinstance(g, KNNGroup) and g.nsample == 16 and g.relative_xyz and not g.normalize_dp
    g = create_grouper({'NAME': 'knn', 'nsample': 8, 'radius': 0.1, 'normalize_dp': True, 'relative_xyz': False})
    assert isinstance(g, KNNGroup) and g.normalize_dp and not g.relative_xyz
    assert isinstance(create_grouper({'NAME': 'ballquery', 'radius': 0.1, 'nsample': 16}), QueryAndGroup)


def test_names_exported():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from openpoints.models import layers
    from openpoints.models.layers import knn, group
    assert layers.knn_point is knn.knn_point and layers.KNN is knn.KNN and layers.DilatedKNN is knn.DilatedKNN
    assert layers.DenseDilated is knn.DenseDilated and layers.KNNGroup is group.KNNGroup
    for name in ("KNN", "DenseDilated", "DilatedKNN", "KNNGroup"):
        assert hasattr(group, name), name


def test_shapes_dtypes_values(fix):
    from openpoints.models.layers import knn, group
    qry, sup = fix["qry"], fix["sup"]
    ok = _agree(fix["knn_idx"], fix["exact"][..., :9])
    for got, val, idx in ((knn.knn_point(9, qry, sup), "point_val", "point_idx"), (knn.KNN(9)(qry, sup), "knn_val", "knn_idx"),
                          (knn.KNN(9, farthest=True)(qry, sup), "far_val", "far_idx")):
        assert got[0].shape == fix[val].shape == (2, 77, 9) and got[1].shape == (2, 77, 9)
        assert str(got[1].dtype) == str(fix[idx + "_dtype"]) and got[0].dtype == torch.float32
        np.testing.assert_allclose(got[0].numpy(), fix[val], rtol=0, atol=4e-7)  # the same composition; 2 ulp of values <= 2
        sel = ok if "far" not in idx else torch.ones_like(ok)
        np.testing.assert_array_equal(got[1][sel].numpy(), fix[idx][sel.numpy()])
    v, i = group.KNN(9)(sup, qry)
    assert v.shape == (2, 9, 77) and i.shape == (2, 77, 9) and i.dtype == torch.int32 and str(fix["gknn_idx_dtype"]) == "torch.int32"
    np.testing.assert_allclose(v.numpy(), fix["gknn_val"], rtol=0, atol=4e-7)
    np.testing.assert_array_equal(i[ok].numpy(), fix["gknn_idx"][ok.numpy()])
    with pytest.raises(RuntimeError):
        knn.KNN(301)(qry, sup)


@pytest.mark.parametrize("tag", ["knn", "group"])
def test_dilated_and_stochastic_pick(fix, tag):
    import openpoints.models.layers as layers
    mod = getattr(layers, tag)
    sup = fix["sup"]
    exact, _ = R.exact_knn(18, sup, sup)
    ok = _agree(torch.from_numpy(fix[f"dil_{tag}"]), exact[..., ::2])
    got = mod.DilatedKNN(9, 2)(sup)
    assert got.shape == (2, 300, 9) and got.dtype == torch.int32 and got.is_contiguous()
    np.testing.assert_array_equal(got[ok].numpy(), fix[f"dil_{tag}"][ok.numpy()])
    seed = int(fix["meta"][8])
    sto = mod.DilatedKNN(9, 2, stochastic=True, epsilon=1.0).train()
    torch.manual_seed(seed)
    got = sto(sup)
    torch.manual_seed(seed)
    torch.rand(1)
    cols = torch.randperm(18)[:9]
    after = torch.rand(1)  # the generator's state after the reference's draws: rand(1), then randperm(18)
    ok = _agree(torch.from_numpy(fix[f"sto_{tag}"]), exact[..., cols])
    assert got.shape == (2, 300, 9) and got.dtype == torch.int32 and got.is_contiguous()
    np.testing.assert_array_equal(got[ok].numpy(), fix[f"sto_{tag}"][ok.numpy()])  # the pick, index for index
    torch.manual_seed(seed)
    sto(sup)
    assert torch.equal(torch.rand(1), after)  # the same draws in the same order
    torch.manual_seed(seed)
    assert torch.equal(sto.eval()(sup), mod.DilatedKNN(9, 2)(sup))  # not training: the strided pick ...
    torch.manual_seed(seed)
    sto(sup)
    first = torch.rand(1)
    torch.manual_seed(seed)
    torch.rand(1)
    assert torch.equal(torch.rand(1), first)  # ... after rand(1) alone


@pytest.mark.parametrize("rel", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
def test_knn_group_cpu_route(fix, rel, norm):
    from openpoints.models.layers.group import KNNGroup
    qry, sup, feat = fix["qry"], fix["sup"], fix["feat"]
    ok = _agree(fix["only_idx"], fix["exact"][..., :9])
    assert bool(ok.all())  # 300 / 77: the reference's lists are exact, so whole tensors compare
    g = KNNGroup(9, relative_xyz=bool(rel), normalize_dp=bool(norm))
    dp, fj = g(qry, sup, feat)
    want = fix[f"dp_r{rel}_n{norm}"]
    assert dp.shape == want.shape == (2, 3, 77, 9) and fj.shape == (2, 5, 77, 9)
    ulp = R.ulp_diff(dp.numpy(), want)
    print("dp differs from the fixture by", ulp, "ulp")
    assert ulp <= (2 if norm else 0)  # gather and subtraction are exact; the divisor and the quotient round once each
    np.testing.assert_array_equal(fj.numpy(), fix["fj"])
    dp2, none = g(qry, sup)
    assert none is None and torch.equal(dp2, dp)
    idx = KNNGroup(9, return_only_idx=True)(qry, sup, feat)
    assert idx.dtype == torch.int32 and str(fix["only_idx_dtype"]) == "torch.int32"
    np.testing.assert_array_equal(idx.numpy(), fix["only_idx"])
    # the helper the GPU tests compare against is the same arithmetic
    hdp, hfj = R.knn_group_forward(idx, qry, sup, feat, bool(rel), bool(norm))
    assert R.ulp_diff(hdp.numpy(), want) <= (2 if norm else 0) and torch.equal(hfj, fj)
    # query() / relative_positions() / geom: QueryAndGroup's protocol
    geom = {"idx": g.query(qry, sup), "dp": g.relative_positions(idx, qry, sup)}
    dp3, fj3 = g(qry, sup, feat, geom=geom)
    assert torch.equal(dp3, dp) and torch.equal(fj3, fj)


def test_self_search_2048_against_fixture(fix):
    from openpoints.models.layers import knn
    big = fix["big"]
    exact, _ = R.exact_knn(16, big, big)
    ok = _agree(torch.from_numpy(fix["big_idx"].astype(np.int64)), exact)
    _, idx = knn.KNN(16)(big)
    np.testing.assert_array_equal(idx[ok].numpy(), fix["big_idx"][ok.numpy()])


@pytest.mark.parametrize("kind,seed", [("uniform", 10), ("room", 9)])
@pytest.mark.parametrize("n,m,k", [(2048, None, 16), (2049, None, 32), (6000, 700, 36), (300, 77, 9), (64, 7, 64)])
def test_oracle_lists_are_the_exact_lists(kind, seed, n, m, k):
    """the yardstick of the GPU tests: on clouds without ties the oracle's lists are the nearest points, every query"""
    sup = torch.from_numpy(clouds(seed, 2, n, kind))
    qry = sup if m is None else torch.from_numpy(clouds(seed + 1, 2, m, kind))
    want, untied = R.exact_knn(k, qry, sup)
    got, _ = R.oracle_knn(k, qry, sup)
    fp32_untied = R.oracle_untied(k, qry, sup)
    sel = untied & fp32_untied
    differ = int((got.long() != want).any(-1)[sel].sum())
    print(f"{differ} of {int(sel.sum())} untied queries differ ({int((~sel).sum())} tied)")
    assert differ == 0 and float(sel.float().mean()) >= 0.99


def test_plan_key_separates_groupers():
    import amcontrast3d_amd
    amcontrast3d_amd.activate()
    from amcontrast3d_amd.geometry import plan_key
    from openpoints.models.layers.group import KNNGroup, QueryAndGroup

    class Ball(QueryAndGroup):  # a ball query whose other key parts equal the k-NN grouper's
        radius = None

    knn_a, knn_b = KNNGroup(16), KNNGroup(16, normalize_dp=False)
    ball = QueryAndGroup(0.1, 16)
    assert plan_key(knn_a) == plan_key(knn_b) and plan_key(knn_a) != plan_key(ball)
    assert plan_key(QueryAndGroup(0.1, 16)) == plan_key(ball) != plan_key(QueryAndGroup(0.2, 16))
    odd = Ball(0.1, 16)
    odd.radius = None
    assert plan_key(odd)[1:] == plan_key(knn_a)[1:] and plan_key(odd) != plan_key(knn_a)
